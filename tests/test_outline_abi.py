"""The selection outline, the part that needs no GPU: gsr_set_overlay_outline is exported by the library, prototyped by the Python
host and declared and documented in include/gsplat_hip.h; gsr_outline_options is 48 bytes with the header's fields; the kernels are
in the code object and in the bounds-checked twin; the C++ caller lists its option; gsr_overlay_options is what it was."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")


def test_symbol_is_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    assert hasattr(lib, "gsr_set_overlay_outline") and "gsr_set_overlay_outline" in gh.EXPORTS
    assert lib.gsr_set_overlay_outline.argtypes == [ctypes.c_void_p, ctypes.POINTER(gh.GsrOutlineOptions)]
    assert lib.gsr_set_overlay_outline.restype is ctypes.c_int
    assert lib.gsr_set_overlay_outline(None, None) == -1            # a NULL context is refused before anything is touched


def test_struct_is_48_bytes_with_the_headers_fields():
    import gsplat_hip as gh
    S = gh.GsrOutlineOptions
    assert ctypes.sizeof(S) == 48
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("rgb", 0, 12), ("alpha", 12, 4), ("threshold", 16, 4), ("width", 20, 4), ("side", 24, 4), ("reserved", 28, 20)]
    assert gh.OUTLINE_SIDES == {"outer": 0, "inner": 1}
    # the overlay's own options are what they were
    assert ctypes.sizeof(gh.GsrOverlayOptions) == 32


def test_header_declares_and_documents_it():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("typedef struct gsr_outline_options { float rgb[3]; float alpha; float threshold; int32_t width; int32_t side; int32_t reserved[5]; } gsr_outline_options;",
                 "int gsr_set_overlay_outline(gsr_ctx *ctx, const gsr_outline_options *options);",
                 "#define GSR_OUTLINE_OUTER 0", "#define GSR_OUTLINE_INNER 1",
                 "typedef struct gsr_overlay_options { float tint[3]; float mix; int32_t reserved[4]; } gsr_overlay_options;"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- selection outline ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on the selection outline"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    for words in ("inside(p) = (cover[p] >= threshold)", "a NaN is not inside", "neither inside nor outside", "never written",
                  "(qx-px)^2 + (qy-py)^2 <= r*r", "inside and !inside exchanged", "k = 1.0f - alpha", "out.c = fma(ov.c, k, rgb[c] * alpha)",
                  "out.a = fma(ov.a, k, alpha)", "out = ov bit for bit", "cover is never changed", "its own bin columns",
                  "did not fit draws nothing", "gsr_set_overlay first", "alpha in [0, 1]", "finite and > 0", "width in 1 .. 16", "reserved 0",
                  "nothing changes", "NULL: off", "make the image stale", "equal options do not", "gsr_set_overlay(ctx, NULL) clears the outline too",
                  "gsr_read_overlay_rgba8", "gsr_overlay_device_ptr(ctx, 0)", "gsr_delivery_set_overlay", "launch for launch"):
        assert words in doc, words


def test_python_host_has_the_method():
    import gsplat_hip as gh
    sig = inspect.signature(gh.HIPRenderer.set_overlay_outline)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("rgb", (1.0, 1.0, 1.0)), ("alpha", 1.0), ("threshold", 0.5), ("width", 2), ("side", "outer")]
    assert list(inspect.signature(gh.HIPRenderer.set_overlay).parameters) == ["self", "tint", "mix"]      # unchanged


def test_kernels_are_in_the_unit_behind_the_pass_and_checked():
    src = open(os.path.join(CSRC, "k_overlay.hip")).read()
    for word in ("void k_outline_bits(OutlineArgs a)", "void k_outline_apply(OutlineArgs a)", "__ballot(source)", "if (*a.invalid != 0u) return;",
                 "__builtin_amdgcn_readfirstlane", "GSR_BOUND(overlay, 6,", "GSR_BOUND(overlay, 7,"):
        assert word in src, word
    assert src.count("if (*a.invalid != 0u) return;") == 2                 # both kernels leave a refused frame alone
    host = open(os.path.join(CSRC, "gsr_overlay.cpp")).read()
    assert "launch_outline(a, c->stream)" in host and "const bool outline = o.outline.on && sc.sel.mask;" in host     # enqueued only when an outline is set
    assert host.index("outline_ensure(c)) return r;") < host.index("launch_overlay(b, g,") < host.index("if (outline) outline_enqueue(c, g);")   # what can fail comes first


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_outline_bitsENS_11OutlineArgsE", "k_outline_applyENS_11OutlineArgsE", "gsr_set_overlay_outline"):
        assert k in out, k
    p = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
    assert os.path.exists(p), p
    t = subprocess.run(["strings", "-a", p], capture_output=True, text=True).stdout
    assert "k_outline_applyENS_11OutlineArgsE" in t and "gsr_debug_bounds_overlay" in t


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--outline WIDTH]" in r.stdout + r.stderr
    r = subprocess.run([exe, "--outline", "2"], capture_output=True, text=True)       # alone it would time nothing: refused
    assert r.returncode == 2 and "--outline WIDTH goes beside --overlay FRACTION" in r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_set_overlay_outline", "gsr_outline_options", "outline_width"):
        assert word in src, word


def test_documents_describe_the_outline():
    for name, words in (("README.md", ("set_overlay_outline", "setSelectionOutline", "gsr_set_overlay_outline")),
                        ("DESIGN.md", ("k_outline_bits", "k_outline_apply", "gsr_set_overlay_outline", "tests/test_gpu_outline.py"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
