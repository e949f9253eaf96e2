"""Shared scenes, the part that needs no GPU: the two entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_abi.py holds the rest of the ABI to the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
NAMES = ("gsr_share_scene", "gsr_scene_sharing")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
    vp = ctypes.c_void_p
    assert lib.gsr_share_scene.argtypes == [vp, vp] and lib.gsr_share_scene.restype is ctypes.c_int
    assert lib.gsr_scene_sharing.argtypes == [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]
    assert lib.gsr_scene_sharing.restype is ctypes.c_int


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+gsr_share_scene\s*\(\s*gsr_ctx\s*\*\s*ctx\s*,\s*gsr_ctx\s*\*\s*from\s*\)\s*;", code)
    assert re.search(r"int\s+gsr_scene_sharing\s*\(\s*gsr_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*members\s*,\s*uint64_t\s*\*\s*scene_bytes\s*\)\s*;", code)
    m = re.search(r"/\* ---- shared scenes.*?\*/", src, flags=re.S)
    assert m, "the header has no section on shared scenes"
    doc = " ".join(m.group(0).split())
    # what is shared, what stays, leaving, SH, edits and their ordering, limitBox, errors, threads
    for words in ("hold once", "stays with each context", "no leader", "Leaving", "still sharing", "gsr_set_scene_sh", "between frames",
                  "no host wait", "one event per other member", "gsr_scene_limit_box", "GSR_ERR_ARG", "different devices",
                  "delivered frame", "gsr_read_scene"):
        assert words in doc, words
    assert "share a scene" in " ".join(src[:src.index("#ifndef")].split())   # the thread rule at the top of the header


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    assert callable(gh.HIPRenderer.share_scene) and callable(gh.HIPRenderer.scene_sharing)
