"""Depth in a group (gsr_comm_set_depth) on a box without a GPU: the header declares the four entry points, the ctypes mirror
matches, the built library exports them and holds the kernels, the hosts name them, the documents describe them."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_ERR_ARG = -1
NAMES = ("gsr_comm_set_depth", "gsr_frame_depth_layout", "gsr_read_frame_depth", "gsr_frame_depth_device_ptr")


def _header():
    return open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()


def test_header_declares_the_four_functions():
    src = _header()
    assert re.search(r"int gsr_comm_set_depth\(gsr_ctx \*ctx, const gsr_depth_delivery_options \*depth\);", src)
    assert re.search(r"int gsr_frame_depth_layout\(gsr_ctx \*ctx, gsr_depth_layout \*out\);", src)
    assert re.search(r"int gsr_read_frame_depth\(gsr_ctx \*ctx, void \*out, uint64_t out_bytes\);", src)
    assert re.search(r"void \*gsr_frame_depth_device_ptr\(gsr_ctx \*ctx\);", src)
    # declared behind the structs they take
    assert src.index("} gsr_depth_layout;") < src.index("int gsr_comm_set_depth(")
    # the two refusals of a context that does not opt in are still described
    assert "unless the context opts in" in src


def test_ctypes_mirror_matches():
    import gsplat_hip as gh
    L = gh.load_library()
    vp = ctypes.c_void_p
    for name in NAMES:
        assert name in gh.EXPORTS, name
    assert L.gsr_comm_set_depth.argtypes == [vp, ctypes.POINTER(gh.GsrDepthDeliveryOptions)]
    assert L.gsr_frame_depth_layout.argtypes == [vp, ctypes.POINTER(gh.GsrDepthLayout)]
    assert L.gsr_read_frame_depth.argtypes == [vp, vp, ctypes.c_uint64]
    assert L.gsr_frame_depth_device_ptr.argtypes == [vp] and L.gsr_frame_depth_device_ptr.restype is vp
    # the structs the new calls share with the depth ring keep their size
    assert ctypes.sizeof(gh.GsrDepthDeliveryOptions) == 16 and ctypes.sizeof(gh.GsrDepthLayout) == 48


def test_library_exports_them_and_refuses_a_null_context():
    import gsplat_hip as gh
    L = gh.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", gh.LIB_PATH], capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
    depth = gh.GsrDepthDeliveryOptions(gh.GSR_DEPTH_U16, 2, 0.1, 0)
    lay = gh.GsrDepthLayout()
    lay.bytes = 77
    buf = (ctypes.c_uint8 * 16)()
    assert L.gsr_comm_set_depth(None, ctypes.byref(depth)) == GSR_ERR_ARG
    assert L.gsr_comm_set_depth(None, None) == GSR_ERR_ARG
    assert L.gsr_frame_depth_layout(None, ctypes.byref(lay)) == GSR_ERR_ARG and lay.bytes == 77
    assert L.gsr_read_frame_depth(None, buf, 16) == GSR_ERR_ARG
    assert L.gsr_frame_depth_device_ptr(None) is None


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr17k_pack_band_depthILi[12]EEEv\w*", out))) == 2
    assert len(set(re.findall(r"_ZN3gsr20k_unpack_slabs_depthILi[12]EEEv\w*", out))) == 2


def test_python_host_names_them():
    import gsplat_hip as gh
    sig = inspect.signature(gh.HIPRenderer.set_group_depth)
    assert list(sig.parameters) == ["self", "depth", "depth_step", "near"]
    assert sig.parameters["depth"].default == "u16" and sig.parameters["depth_step"].default == 1 and sig.parameters["near"].default == 0.1
    for name in ("frame_depth_layout", "read_frame_depth"):
        assert name in gh.HIPRenderer.__dict__, name


def test_node_host_names_them():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    assert re.search(r"\bsetGroupDepth\(depth: DepthDeliveryOptions \| null\): void", dts)
    assert re.search(r"\breadFrameDepth\(\): Uint16Array \| Float32Array", dts)
    assert re.search(r"\bframeDepthLayout\(\): DepthLayout", dts)
    js = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    assert "this.setGroupDepth =" in js and "this.readFrameDepth =" in js and "g.depth" in js
    addon_src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for entry in ('{"commSetDepth", CommSetDepth}', '{"frameDepthLayout", FrameDepthLayout}', '{"readFrameDepth", ReadFrameDepth}'):
        assert entry in addon_src, entry
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    if os.path.exists(addon):                                  # (built only where the Node headers are)
        out = subprocess.run(["strings", "-a", addon], capture_output=True, text=True).stdout
        for name in ("commSetDepth", "readFrameDepth", "gsr_comm_set_depth", "gsr_read_frame_depth"):
            assert name in out, name


def test_documents_describe_the_exchange():
    for name, words in (("README.md", ("gsr_comm_set_depth", "set_group_depth", "setGroupDepth")),
                        ("DESIGN.md", ("Depth in a group", "k_pack_band_depth", "k_unpack_slabs_depth", "gsr_comm_set_depth")),
                        ("INTEGRATION.md", ("gsr_comm_set_depth",))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
