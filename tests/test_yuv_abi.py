"""The Y'CbCr side of the delivery ring on a box without a GPU: the header declares it, the library exports it, the hosts name
it, the kernel is in the gfx950 code object, and the tools that need a GPU say so."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()


def test_header_declares_formats_structs_and_entry_points():
    import gsplat_hip as gh
    src = _header()
    for name, value in (("RGBA8", 0), ("NV12", 1), ("I420", 2)):
        assert re.search(r"#define GSR_FORMAT_%s\s+%d\b" % (name, value), src), name
        assert getattr(gh, "GSR_FORMAT_" + name) == value
    assert gh.DELIVERY_FORMATS == {"rgba8": 0, "nv12": 1, "i420": 2}
    assert re.search(r"int gsr_delivery_open_ex\(gsr_ctx \*ctx, const gsr_delivery_options \*opt\);", src)
    assert re.search(r"int gsr_delivery_layout\(gsr_ctx \*ctx, gsr_frame_layout \*out\);", src)
    for struct, mirror in (("gsr_delivery_options", gh.GsrDeliveryOptions), ("gsr_frame_layout", gh.GsrFrameLayout)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.split(None, 1)[1])]
        assert fields == [n for n, _ in mirror._fields_], struct
    assert ctypes.sizeof(gh.GsrDeliveryOptions) == 16 and gh.GsrDeliveryOptions.background.offset == 12
    assert ctypes.sizeof(gh.GsrFrameLayout) == 72 and gh.GsrFrameLayout.offset.offset == 16 and gh.GsrFrameLayout.bytes.offset == 64
    assert ctypes.sizeof(gh.GsrFrame) == 32                    # the frame itself is unchanged


def test_library_exports_them_and_refuses_a_null_context():
    import gsplat_hip as gh
    L = gh.load_library()
    assert "gsr_delivery_open_ex" in gh.EXPORTS and "gsr_delivery_layout" in gh.EXPORTS
    opt = gh.GsrDeliveryOptions(3, gh.GSR_FORMAT_NV12, 0, (ctypes.c_uint8 * 4)(0, 0, 0, 0))
    lay = gh.GsrFrameLayout()
    lay.bytes = 77
    assert L.gsr_delivery_open_ex(None, ctypes.byref(opt)) == GSR_ERR_ARG
    assert L.gsr_delivery_open_ex(None, None) == GSR_ERR_ARG
    assert L.gsr_delivery_layout(None, ctypes.byref(lay)) == GSR_ERR_ARG and lay.bytes == 77


def test_python_host_names_them():
    import gsplat_hip as gh
    sig = inspect.signature(gh.HIPRenderer.open_delivery)
    assert list(sig.parameters) == ["self", "slots", "format", "full_range", "background"]
    assert sig.parameters["slots"].default == 3 and sig.parameters["format"].default == "rgba8"
    assert sig.parameters["full_range"].default is False and tuple(sig.parameters["background"].default) == (0, 0, 0)
    assert "delivery_layout" in gh.HIPRenderer.__dict__


def test_node_host_names_them():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    cls = dts[dts.index("export class HIPRenderer"):]
    cls = cls[:cls.index("\n}")]
    assert re.search(r"openDelivery\(slots\?: number, options\?: DeliveryOptions\)", cls) and re.search(r"\bdeliveryLayout\(\)", cls)
    opts = dts[dts.index("export interface DeliveryOptions"):]
    opts = opts[:opts.index("\n}")]
    for field in ("format?: DeliveryFormat", "fullRange?: boolean", "background?:"):
        assert field in opts, field
    assert re.search(r'export type DeliveryFormat = "rgba8" \| "nv12" \| "i420";', dts)
    frame = dts[dts.index("export interface DeliveredFrame"):]
    frame = frame[:frame.index("\n}")]
    for field in ("pixels: Uint8Array", "format: DeliveryFormat", "planes: DeliveredPlane[]"):
        assert field in frame, field
    js = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    assert re.search(r"this\.openDelivery = \(slots, options\)", js) and re.search(r"this\.deliveryLayout\s*=", js)
    addon_src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    assert '{"openDeliveryEx", OpenDeliveryEx}' in addon_src and '{"deliveryLayout", DeliveryLayout}' in addon_src
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    if os.path.exists(addon):                                  # (built only where the Node headers are)
        out = subprocess.run(["strings", "-a", addon], capture_output=True, text=True).stdout
        for name in ("openDeliveryEx", "deliveryLayout", "gsr_delivery_open_ex", "gsr_delivery_layout"):
            assert name in out, name


def test_library_holds_the_yuv_kernel():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out and "k_deliver_yuv" in out and "k_deliver_rgba8" in out
    # two formats x two sources
    assert len(set(re.findall(r"_ZN3gsr13k_deliver_yuvILi[12]E\w*?EEvPKT0_", out))) == 4


def test_cpp_caller_lists_the_formats():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--deliver-format nv12|i420" in r.stdout + r.stderr
    r = subprocess.run([exe, "--deliver", "--deliver-format", "yuv9"], capture_output=True, text=True)
    assert r.returncode == 2 and "nv12|i420" in r.stderr


def test_bench_delivery_format_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_yuv_delivery.py runs the script")
    script = os.path.join(ROOT, "scripts", "bench_delivery.py")
    r = subprocess.run([sys.executable, script, "--config", "C1", "--format", "nv12"], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU path" in r.stderr
    r = subprocess.run([sys.executable, script, "--format", "yuv9"], capture_output=True, text=True)
    assert r.returncode != 0 and "invalid choice" in r.stderr
