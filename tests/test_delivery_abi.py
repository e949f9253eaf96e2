"""The delivery entry points of the C ABI on a box without a GPU: every one of them answers a NULL context with
GSR_ERR_ARG (gsr_delivery_slot_ptr: NULL and 0 bytes), the struct the hosts mirror has the header's layout, and the
conversion kernel is in the library's gfx950 code object."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_ERR_ARG = -1


def test_every_delivery_entry_point_refuses_a_null_context():
    import gsplat_hip as gh
    L = gh.load_library()
    k = ctypes.c_uint64(77)
    f = gh.GsrFrame()
    nbytes = ctypes.c_uint64(77)
    assert L.gsr_delivery_open(None, 3) == GSR_ERR_ARG
    assert L.gsr_delivery_close(None) == GSR_ERR_ARG
    assert L.gsr_deliver_frame_async(None, ctypes.byref(k)) == GSR_ERR_ARG and k.value == 77
    assert L.gsr_frame_ready(None, 1) == GSR_ERR_ARG
    assert L.gsr_acquire_frame(None, 1, ctypes.byref(f)) == GSR_ERR_ARG and not f.pixels
    assert L.gsr_release_frame(None, 1) == GSR_ERR_ARG
    assert L.gsr_delivery_slot_ptr(None, 0, ctypes.byref(nbytes)) is None and nbytes.value == 0
    assert L.gsr_delivery_slot_ptr(None, 0, None) is None


def test_header_declares_the_ring_and_the_hosts_mirror_it():
    import gsplat_hip as gh
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define GSR_ERR_BUSY \(-7\)", src) and gh.GSR_ERR_BUSY == -7
    body = re.search(r"typedef struct gsr_frame \{(.*?)\} gsr_frame;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "")]
    assert fields == [n for n, _ in gh.GsrFrame._fields_]
    assert ctypes.sizeof(gh.GsrFrame) == 32 and gh.GsrFrame.serial.offset == 24
    r = gh.HIPRenderer.__dict__
    for m in ("open_delivery", "close_delivery", "deliver", "frame_ready", "acquire", "release"):
        assert m in r


def test_cpp_caller_has_a_deliver_leg():
    # (what it delivers is checked on the GPU: tests/test_gpu_delivery.py, where a live but ring-less context is refused too)
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--deliver" in r.stdout + r.stderr


def test_library_holds_the_delivery_kernel():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out and "k_deliver_rgba8" in out


def test_bench_delivery_fails_loudly_without_gpu():
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_delivery.py runs the script")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_delivery.py"), "--config", "C1"], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU path" in r.stderr
