"""The selection overlay, the part that needs no GPU: the six entry points are exported by the library, prototyped by the Python host
and documented in include/gsplat_hip.h, the way tests/test_contrib_abi.py holds contribution to the header; the sources are wired
into every build, the kernel is in the code object in its four forms, and the C++ caller lists its option."""
import ctypes
import os
import re
import subprocess

from walk_source import walk_is_stated_once, walk_sites_are_checked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_set_overlay", "gsr_overlay_async", "gsr_read_overlay", "gsr_read_overlay_rgba8", "gsr_overlay_device_ptr", "gsr_delivery_set_overlay")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert lib.gsr_set_overlay.argtypes == [vp, ctypes.POINTER(gh.GsrOverlayOptions)] and lib.gsr_set_overlay.restype is ctypes.c_int
    assert lib.gsr_overlay_async.argtypes == [vp] and lib.gsr_overlay_async.restype is ctypes.c_int
    assert lib.gsr_read_overlay.argtypes == [vp, vp, vp] and lib.gsr_read_overlay.restype is ctypes.c_int
    assert lib.gsr_read_overlay_rgba8.argtypes == [vp, vp] and lib.gsr_read_overlay_rgba8.restype is ctypes.c_int
    assert lib.gsr_overlay_device_ptr.argtypes == [vp, i32] and lib.gsr_overlay_device_ptr.restype is vp
    assert lib.gsr_delivery_set_overlay.argtypes == [vp, i32] and lib.gsr_delivery_set_overlay.restype is ctypes.c_int
    # the options struct is the header's: three floats, a float, four reserved words
    assert ctypes.sizeof(gh.GsrOverlayOptions) == 32
    assert [(n, ctypes.sizeof(t)) for n, t in gh.GsrOverlayOptions._fields_] == [("tint", 12), ("mix", 4), ("reserved", 16)]
    # a NULL context is refused before anything is touched
    for call in (lambda: lib.gsr_set_overlay(None, None), lambda: lib.gsr_overlay_async(None), lambda: lib.gsr_read_overlay(None, None, None),
                 lambda: lib.gsr_read_overlay_rgba8(None, None), lambda: lib.gsr_delivery_set_overlay(None, 1)):
        assert call() == -1
    assert not lib.gsr_overlay_device_ptr(None, 0)


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("typedef struct gsr_overlay_options { float tint[3]; float mix; int32_t reserved[4]; } gsr_overlay_options;",
                 "int gsr_set_overlay(gsr_ctx *ctx, const gsr_overlay_options *options);", "int gsr_overlay_async(gsr_ctx *ctx);",
                 "int gsr_read_overlay(gsr_ctx *ctx, float *rgba , float *cover );", "int gsr_read_overlay_rgba8(gsr_ctx *ctx, uint8_t *out);",
                 "void *gsr_overlay_device_ptr(gsr_ctx *ctx, int32_t plane);", "int gsr_delivery_set_overlay(gsr_ctx *ctx, int32_t on);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- selection overlay ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on the selection overlay"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definition, the two results, each call's rules, the refusals, delivery, shared scenes
    for words in ("exactly those of \"depth and pick\"", "pass q <= 4", "no early termination, no saturation skip and no segments",
                  "(float)byte * (1.0f / 255.0f)", "evaluated SH colour", "w = T * B; T = T - w;", "S = S + w; Cr = fma(w, cr, Cr)",
                  "the share of the pixel's alpha that selected splats supply", "premultiplied like the framebuffer",
                  "out.r = fma(mix, fma(tint[0], S, -Cr), fb.r)", "out.a = fb.a", "lerp(c, tint, mix)", "gives fb bit for bit", "Nothing is clamped here",
                  "its own bin columns", "elsewhere cover is 0", "never writes it", "no host wait beyond what allocating needs", "mix in [0, 1]",
                  "reserved 0", "nothing changes", "NULL: off, the buffers are freed", "scene_bytes does not change",
                  "exactly what gsr_depth_async needs", "nothing is enqueued", "GSR_ERR_ARG also without options", "no mask is allocated",
                  "overflow word", "ever returned as data", "settle the frame as gsr_read_depth does", "this frame, this selection and these options",
                  "GSR_ERR_OVERFLOW", "either may be NULL", "plane 0 the overlay", "1 cover", "in place of the framebuffer",
                  "serials, GSR_ERR_BUSY, the overflow refusal, resize and close behave as before", "a depth ring's plane is still the frame's",
                  "RGBA8 of other ranks", "byte for byte what it does without this call", "gsr_sync clears the note",
                  "first waits for the streams of the members with such a note", "never sees the change", "make the image stale",
                  "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    import inspect
    for name in ("set_overlay", "overlay_async", "read_overlay", "read_overlay_rgba8", "delivery_set_overlay"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    assert list(inspect.signature(gh.HIPRenderer.delivery_set_overlay).parameters) == ["self", "on"]
    assert inspect.signature(gh.HIPRenderer.delivery_set_overlay).parameters["on"].default is True


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_overlay.hip" in srcs and "gsr_overlay.cpp" in srcs        # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id and "k_depth_walk.h" in build_id
    exp = open(os.path.join(ROOT, "scripts", "build_exp.sh")).read()
    assert "make" in exp and "OUT=../lib_exp/$name" in exp             # the bounds and cppwalk twins ARE the csrc Makefile
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"bounds", "-DGSR_BOUNDS"' in entry and '"cppwalk", "-DGSR_CPP_WALK"' in entry
    src = open(os.path.join(CSRC, "k_overlay.hip")).read()
    assert "GSR_BOUNDS_DECL(overlay)" in src
    walk_sites_are_checked(src, "overlay", "OverlayBounds", "OverlayPass")   # bin, list position, splat index, LDS cell: in the walk the unit instantiates
    for site in (4, 5):                                                 # mask word, pixel: the unit's own
        assert re.search(r"GSR_BOUND\(overlay, %d," % site, src), site
    assert "walk_list_entry<OverlayBounds>(a, e)" in src                # the TRIM pass over the list reads it through the same checks
    api = open(os.path.join(CSRC, "gsr_api.cpp")).read()
    assert 'getenv("GSR_OVERLAY_TRIM")' in api and 'getenv("GSR_DEPTH_SKIP")' in api       # read once, where a context is created


def test_the_walk_arithmetic_is_shared_and_the_frame_chain_is_not_touched():
    src = open(os.path.join(CSRC, "k_overlay.hip")).read()
    assert '#include "k_depth_walk.h"' in src
    for fn in ("depth_weight(", "depth_row_u(", "depth_row_w(", "walk_bin_list<SKIP>(st, a, w, cam, w.begin, end, pass)", "walk_frame_unfit(a.overflow, a.invalid)"):
        assert fn in src, fn
    walk_is_stated_once()                           # depth_entry and depth_tile_reach: in the walk's skeleton, for all three units
    assert "exp2f" not in src and "struct DepthEntry" not in src        # used, never restated
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code  and "atomicAdd" not in code         # plain vector stores; the one LDS maximum is a HIP atomic
    for word in ("__ballot", "__hip_atomic_fetch_max", "__HIP_MEMORY_SCOPE_WORKGROUP", "__builtin_fmaf", "RGB8_IN_SHCOL", "a.shcol[i]",
                 "template <bool SKIP, bool TRIM>"):
        assert word in src, word
    # the selection bit as the issue states it
    assert re.search(r"a\.sel\[word\] >> \(i & 31u\)", src) and "i >> 5" in src
    # nothing of the frame chain names the overlay: no branch, no load, no argument
    for name in ("k_project.hip", "k_blend.hip", "k_sort.hip", "k_bin.hip", "k_deliver.hip", "gsr_frame.cpp"):
        assert "overlay" not in open(os.path.join(CSRC, name)).read().lower(), name


def test_library_holds_the_kernel_in_its_four_forms():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr9k_overlayILb[01]ELb[01]EEEvNS_14OverlayBuffersE\w*", out))) >= 4      # tile skip x trim
    for twin in ("bounds", "cppwalk"):
        p = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", twin, "libgsplat_hip.so")
        assert os.path.exists(p), p
        t = subprocess.run(["strings", "-a", p], capture_output=True, text=True).stdout
        assert "k_overlayILb1ELb1EEE" in t and ("gsr_debug_bounds_overlay" in t) == (twin == "bounds"), twin


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--overlay FRACTION]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_selection_set", "gsr_set_overlay", "gsr_overlay_async", "gsr_read_overlay_rgba8", "overlay_pass_us", "overlay_selected",
                 "overlay_rgba8_fnv1a", "overlay_cover_fnv1a"):
        assert word in src, word


def test_documents_describe_the_pass():
    for name, words in (("README.md", ("gsr_overlay_async", "set_overlay", "setSelectionOverlay")),
                        ("DESIGN.md", ("\"Selection overlay\"", "k_overlay", "5.10", "GSR_OVERLAY_TRIM"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
