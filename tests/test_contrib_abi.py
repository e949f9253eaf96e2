"""Contribution, the part that needs no GPU: the four entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_select_abi.py holds selection to the header; the sources are wired into
every build, the kernels are in the code object, and the C++ caller lists its option."""
import ctypes
import os
import re
import subprocess

from walk_source import walk_is_stated_once, walk_sites_are_checked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_contrib_reset", "gsr_contrib_accumulate_async", "gsr_read_contrib", "gsr_select_contrib")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    assert lib.gsr_contrib_reset.argtypes == [vp]
    assert lib.gsr_contrib_accumulate_async.argtypes == [vp]
    assert lib.gsr_read_contrib.argtypes == [vp, vp, vp, vp, u32, u32p]
    assert lib.gsr_select_contrib.argtypes == [vp, i32, ctypes.c_double, i32, u32p]
    assert gh.CONTRIB_STATS == {"weight": 0, "peak": 1, "pixels": 2}


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_CONTRIB_WEIGHT 0", "#define GSR_CONTRIB_PEAK 1", "#define GSR_CONTRIB_PIXELS 2",
                 "int gsr_contrib_reset(gsr_ctx *ctx);", "int gsr_contrib_accumulate_async(gsr_ctx *ctx);",
                 "int gsr_read_contrib(gsr_ctx *ctx, uint64_t *weight, float *peak, uint32_t *pixels, uint32_t n, uint32_t *frames);",
                 "int gsr_select_contrib(gsr_ctx *ctx, int32_t stat, double below, int32_t op, uint32_t *selected);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- contribution ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on contribution"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())             # (the comment's line prefix goes, a product's " * " stays)
    # the definition, the three accumulators and frames, each call's rules, the refusals, where the state lives and what drops it
    for words in ("exactly those of \"depth and pick\"", "pass q <= 4", "w = T * B, then T = T - w", "no early termination, no saturation skip and no segments",
                  "(uint64_t)rintf(w * 16777216.0f)", "quanta of 2^-24", "ties to even", "at most 2^24", "independent of the order",
                  "taken on the bit patterns", "whatever their weight", "wraps modulo 2^32", "since the last reset", "Only pixels of the image count",
                  "sums add, peaks take the maximum", "its own bin columns only", "adding weight and pixels and taking the maximum of peak",
                  "16 bytes per splat row plus the counter words", "waits for every member's stream", "as gsr_set_scene_sh does",
                  "behind the last enqueued frame", "no host wait", "nothing allocated after the first use", "exactly what gsr_depth_async needs",
                  "nothing is enqueued", "does what gsr_contrib_reset does first", "contributes nothing and does not bump frames", "overflow word",
                  "the depth planes and their validity are not touched", "settles the streams that may hold passes", "Any output may be NULL",
                  "n must equal the scene's count", "nothing was ever reset or accumulated", "value_i < below", "compared in f64 on the device over ALL splats",
                  "has value 0", "folded into the selection", "blocking", "an unknown stat or op", "a NaN `below`", "frames == 0",
                  "keeps an empty tour from selecting the whole scene", "beside the selection", "ONE set of accumulators", "agent-scope integer atomics and commute",
                  "scene_bytes counts the buffers once they exist", "_rotate and _scale keep the accumulators", "an erase that removes something",
                  "leaving a share drop them", "\"never reset\"", "sees `from`'s accumulators", "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("contrib_reset", "contrib_accumulate", "read_contrib", "select_contrib"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("resetContribution(", "accumulateContribution(", "readContribution(", "selectContribution("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_contrib.hip" in srcs and "gsr_contrib.cpp" in srcs        # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the bounds build
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id and "k_depth_walk.h" in build_id
    exp = open(os.path.join(ROOT, "scripts", "build_exp.sh")).read()
    assert "make" in exp and "OUT=../lib_exp/$name" in exp
    src = open(os.path.join(CSRC, "k_contrib.hip")).read()
    assert "GSR_BOUNDS_DECL(contrib)" in src
    walk_sites_are_checked(src, "contrib", "ContribBounds", None)   # bin, list position, splat index: in the walk's helpers; LDS cell: in the unit's own loop
    for site in (4, 5):                                                 # accumulator index, selection word: the unit's own
        assert re.search(r"GSR_BOUND\(contrib, %d," % site, src), site


def test_the_walk_arithmetic_is_stated_once():
    walk_is_stated_once()
    src = open(os.path.join(CSRC, "k_contrib.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)                         # vector stores and HIP atomics only
    for word in ("__hip_atomic_fetch_add", "__hip_atomic_fetch_max", "__HIP_MEMORY_SCOPE_AGENT", "__ATOMIC_RELAXED", "__shfl_xor", "rintf("):
        assert word in src, word


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr9k_contribILb[01]EEEvNS_14ContribBuffersE\w*", out))) == 2      # with and without the tile skip
    assert re.search(r"_ZN3gsr16k_contrib_selectE\w+", out)


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--contrib]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_contrib_accumulate_async", "gsr_read_contrib", "contrib_pass_ms", "contrib_frames", "contrib_weight_fnv1a", "contrib_peak_fnv1a",
                 "contrib_pixels_fnv1a"):
        assert word in src, word


def test_documents_describe_the_pass():
    for name, words in (("README.md", ("gsr_contrib_accumulate_async", "select_contrib", "selectContribution")),
                        ("DESIGN.md", ("\"Contribution\"", "k_contrib", "5.8", "accumulators that survive an erase"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
