"""The depth ring (gsr_delivery_open_depth) on a box without a GPU: the header declares it, the library exports it, the hosts
name it, the kernels are in the gfx950 code object, and the tools list their options."""
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


def _struct_fields(src, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.split(None, 1)[1])]


def test_header_declares_defines_structs_and_entry_points():
    import gsplat_hip as gh
    src = _header()
    for name, value in (("NONE", 0), ("F32", 1), ("U16", 2)):
        assert re.search(r"#define GSR_DEPTH_%s\s+%d\b" % (name, value), src), name
        assert getattr(gh, "GSR_DEPTH_" + name) == value
    assert gh.DEPTH_DELIVERY_FORMATS == {"f32": 1, "u16": 2}
    assert re.search(r"int gsr_delivery_open_depth\(gsr_ctx \*ctx, const gsr_delivery_options \*opt, const gsr_depth_delivery_options \*depth\);", src)
    assert re.search(r"int gsr_delivery_depth_layout\(gsr_ctx \*ctx, gsr_depth_layout \*out\);", src)
    for struct, mirror in (("gsr_depth_delivery_options", gh.GsrDepthDeliveryOptions), ("gsr_depth_layout", gh.GsrDepthLayout)):
        assert _struct_fields(src, struct) == [n for n, _ in mirror._fields_], struct
    assert ctypes.sizeof(gh.GsrDepthDeliveryOptions) == 16 and gh.GsrDepthDeliveryOptions.near.offset == 8
    assert ctypes.sizeof(gh.GsrDepthLayout) == 48
    assert gh.GsrDepthLayout.offset.offset == 24 and gh.GsrDepthLayout.bytes.offset == 32 and gh.GsrDepthLayout.near.offset == 40
    # what hosts were compiled against keeps its size
    assert ctypes.sizeof(gh.GsrFrame) == 32 and ctypes.sizeof(gh.GsrDeliveryOptions) == 16 and ctypes.sizeof(gh.GsrFrameLayout) == 72


def test_library_exports_them_and_refuses_a_null_context():
    import gsplat_hip as gh
    L = gh.load_library()
    assert "gsr_delivery_open_depth" in gh.EXPORTS and "gsr_delivery_depth_layout" in gh.EXPORTS
    opt = gh.GsrDeliveryOptions(3, gh.GSR_FORMAT_NV12, 0, (ctypes.c_uint8 * 4)(0, 0, 0, 0))
    depth = gh.GsrDepthDeliveryOptions(gh.GSR_DEPTH_U16, 2, 0.1, 0)
    lay = gh.GsrDepthLayout()
    lay.bytes = 77
    assert L.gsr_delivery_open_depth(None, ctypes.byref(opt), ctypes.byref(depth)) == GSR_ERR_ARG
    assert L.gsr_delivery_open_depth(None, None, None) == GSR_ERR_ARG
    assert L.gsr_delivery_depth_layout(None, ctypes.byref(lay)) == GSR_ERR_ARG and lay.bytes == 77


def test_python_host_names_them():
    import gsplat_hip as gh
    sig = inspect.signature(gh.HIPRenderer.open_delivery_depth)
    assert list(sig.parameters) == ["self", "slots", "format", "full_range", "background", "depth", "depth_step", "depth_near"]
    assert sig.parameters["depth_step"].default == 1 and sig.parameters["depth_near"].default == 0.1 and sig.parameters["format"].default == "rgba8"
    assert "depth_layout" in gh.HIPRenderer.__dict__
    # the ring every caller knows keeps its signature
    assert list(inspect.signature(gh.HIPRenderer.open_delivery).parameters) == ["self", "slots", "format", "full_range", "background"]


def test_node_host_names_them():
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    opts = dts[dts.index("export interface DeliveryOptions"):]
    opts = opts[:opts.index("\n}")]
    assert "depth?: DepthDeliveryOptions" in opts
    dopts = dts[dts.index("export interface DepthDeliveryOptions"):]
    dopts = dopts[:dopts.index("\n}")]
    for field in ("format?: DepthDeliveryFormat", "step?: 1 | 2", "near?: number"):
        assert field in dopts, field
    assert re.search(r'export type DepthDeliveryFormat = "f32" \| "u16";', dts)
    frame = dts[dts.index("export interface DeliveredFrame"):]
    frame = frame[:frame.index("\n}")]
    assert "depth?: Uint16Array | Float32Array" in frame and "depthLayout?: DepthLayout" in frame
    assert re.search(r"\bdepthLayout\(\): DepthLayout", dts)
    js = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    assert "openDeliveryDepth(" in js and re.search(r"this\.depthLayout\s*=", js) and "new Uint16Array(b, d.offset" in js
    addon_src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    assert '{"openDeliveryDepth", OpenDeliveryDepth}' in addon_src and '{"depthLayout", DepthLayout}' in addon_src
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    if os.path.exists(addon):                                  # (built only where the Node headers are)
        out = subprocess.run(["strings", "-a", addon], capture_output=True, text=True).stdout
        for name in ("openDeliveryDepth", "depthLayout", "gsr_delivery_open_depth", "gsr_delivery_depth_layout"):
            assert name in out, name


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    # both formats of the conversion
    assert len(set(re.findall(r"_ZN3gsr15k_deliver_depthILi[12]EEEv\w*", out))) == 2
    # the planes pass: with and without the skip, at both steps
    assert len(set(re.findall(r"_ZN3gsr14k_depth_planesILb[01]ELi[12]EEEvNS_12DepthBuffersE\w*", out))) == 4


def test_cpp_caller_lists_the_options():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    for option in ("--deliver-depth f32|u16", "--depth-step 1|2", "--depth-near X"):
        assert option in r.stdout + r.stderr, option
    r = subprocess.run([exe, "--deliver", "--deliver-depth", "u8"], capture_output=True, text=True)
    assert r.returncode == 2 and "f32|u16" in r.stderr
    r = subprocess.run([exe, "--deliver-depth", "u16"], capture_output=True, text=True)
    assert r.returncode == 2 and "--deliver" in r.stderr


def test_bench_delivery_names_the_options():
    script = os.path.join(ROOT, "scripts", "bench_delivery.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for option in ("--depth {f32,u16}", "--depth-step {1,2}", "--depth-near"):
        assert option in r.stdout, option
    r = subprocess.run([sys.executable, script, "--depth", "u8"], capture_output=True, text=True)
    assert r.returncode != 0 and "invalid choice" in r.stderr
    r = subprocess.run([sys.executable, script, "--depth", "u16", "--depth-step", "4"], capture_output=True, text=True)
    assert r.returncode != 0 and "invalid choice" in r.stderr


def test_documents_describe_the_ring():
    for name, words in (("README.md", ("gsr_delivery_open_depth", "open_delivery_depth")), ("DESIGN.md", ("Frame delivery with depth", "k_deliver_depth")),
                        ("INTEGRATION.md", ("gsr_delivery_open_depth",))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
