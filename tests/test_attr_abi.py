"""Splat data, the part that needs no GPU: the three entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_contrib_abi.py holds contribution to the header; the sources are wired into
every build, the value of an attribute is stated once, the kernels are in the code object, and the C++ caller lists its option."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_attr_stats", "gsr_attr_histogram", "gsr_select_attr")
CODES = ("X", "Y", "Z", "DISTANCE", "RED", "GREEN", "BLUE", "OPACITY", "SCALE_X", "SCALE_Y", "SCALE_Z", "SCALE_MIN", "SCALE_MAX",
         "CONTRIB_WEIGHT", "CONTRIB_PEAK", "CONTRIB_PIXELS")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_double
    u32p, f64p = ctypes.POINTER(u32), ctypes.POINTER(f64)
    assert lib.gsr_attr_stats.argtypes == [vp, i32, vp, u32, u32p, u32p, f64p, f64p]
    assert lib.gsr_attr_histogram.argtypes == [vp, i32, vp, u32, f64, f64, u32, vp, vp]
    assert lib.gsr_select_attr.argtypes == [vp, i32, vp, f64, f64, i32, u32p]
    assert gh.ATTRS == {name.lower(): k for k, name in enumerate(CODES)}
    assert gh.SCOPES == {"selected": 1, "visible": 2}


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for k, name in enumerate(CODES):
        assert "#define GSR_ATTR_%s %d" % (name, k) in flat, name
    for decl in ("#define GSR_SCOPE_SELECTED 1u", "#define GSR_SCOPE_VISIBLE 2u",
                 "int gsr_attr_stats(gsr_ctx *ctx, int32_t attr, const double *origin, uint32_t scope, uint32_t *count, uint32_t *nan, double *min, double *max);",
                 "int gsr_attr_histogram(gsr_ctx *ctx, int32_t attr, const double *origin, uint32_t scope, double lo, double hi, uint32_t bins, uint32_t *counts, uint32_t *outside);",
                 "int gsr_select_attr(gsr_ctx *ctx, int32_t attr, const double *origin, double lo, double hi, int32_t op, uint32_t *selected);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- splat data ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on splat data"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())             # (the comment's line prefix goes, a product's " * " stays)
    # the table, the edge rule, the consistency guarantee, the scopes, the calls' rules and the refusals
    for words in ("sqrt((dx*dx + dy*dy) + dz*dz)", "correctly rounded", "numbered as gsr_scene_set_rgba_selected numbers them", "opacity the top byte",
                  "NaN if any scale component is NaN", "exactly the value gsr_select_contrib compares", "ignored otherwise",
                  "GSR_SCOPE_SELECTED counts only splats in the selection", "only splats not in the hidden set", "the flags combine",
                  "infinities included", "-0.0 and 0.0 are equal", "min is +inf and max is -inf", "Any out pointer may be NULL", "An empty scene returns zeros",
                  "1 <= bins <= 4096", "hi - lo finite", "w = (hi - lo) / (double)bins", "edge(k) = k == bins ? hi : min(lo + (double)k * w, hi)",
                  "nondecreasing", "edge(0) == lo", "lo <= v && v < hi", "the largest b < bins with edge(b) <= v", "not by floor((v - lo) / w)",
                  "v < lo, with v >= hi, and with a NaN value", "sum(counts) + sum(outside) == count", "a NaN value is never picked", "lo == hi picks nothing",
                  "hidden ones included", "The consistency guarantee", "for 0 <= a < b <= bins", "gsr_select_attr(attr, origin, edge(a), edge(b), GSR_SELOP_REPLACE)",
                  "exactly sum(counts[a .. b-1]) splats of a scope-0 gsr_attr_histogram", "what the histogram shows is what the range selects",
                  "blocking", "ordered like gsr_select_contrib", "wait for every member's stream", "write none of it",
                  "an unknown attribute code", "a NULL origin or a non-finite origin component", "as gsr_scene_scale_selected refuses",
                  "as gsr_select_contrib refuses", "frames == 0", "a NaN bound or lo > hi", "belong to the context", "allocated by the first call",
                  "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("attr_stats", "attr_histogram", "select_attr"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    assert callable(gh.attr_edges)
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("splatStats(", "splatHistogram(", "selectAttribute("):
        assert name in dts, name


def _ops_body(start, end):
    """k_splat_ops.h between two of its functions' names, comments dropped"""
    ops = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_splat_ops.h")).read())
    return ops[ops.index(start):ops.index(end)]


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_attr.hip" in srcs and "gsr_attr.cpp" in srcs              # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the bounds build
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id and "k_attr.h" in build_id
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(CSRC, "k_attr.hip")).read()
    assert "GSR_BOUNDS_DECL(attr)" in src
    for site in range(6):                                               # set word, splat index, LDS counter, global counter, partial slot, selection word
        assert re.search(r"GSR_BOUND\(attr, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                            # vector stores and HIP atomics only
    for word in ("__hip_atomic_fetch_add", "lds_counters_flush<attr_sites>(", "__HIP_MEMORY_SCOPE_WORKGROUP", "__ATOMIC_RELAXED", "__ballot", "in_scope<attr_sites>(",
                 "extern __shared__"):
        assert word in code, word
    # the scope reads the sets through set_word and the flush is agent-scope atomics: k_splat_ops.h, for every unit
    assert "set_word(" in _ops_body("uint32_t scope_word(", "bool in_scope(")
    assert "__HIP_MEMORY_SCOPE_AGENT" in _ops_body("void lds_counters_flush(", "void workgroup_sum_u64(")
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)", code)    # integer atomics only; min / max go through partials


def test_the_value_is_stated_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp"))}
    with_expr = lambda pat: [f for f, text in files.items() if re.search(pat, re.sub(r"//.*", "", text))]
    assert with_expr(re.escape("(1.0 / 16777216.0)")) == ["k_attr.h"]           # the contribution weight's value: no longer in k_contrib.hip
    assert with_expr(r"__uint_as_float\(\w*\.?peak\[i\]\)") == ["k_attr.h"]
    assert with_expr(r"__device__[^;{]*\battr_value\(") == ["k_attr.h"]
    assert with_expr(re.escape("(dx * dx + dy * dy) + dz * dz")) == ["k_attr.h"]
    users = with_expr(r"\battr_value\(")
    assert users == ["k_attr.h", "k_attr.hip", "k_contrib.hip"], users
    for f in ("k_attr.hip", "k_contrib.hip"):
        assert '#include "k_attr.h"' in files[f], f
    assert files["k_attr.hip"].count("attr_value(") >= 3                        # stats, histogram and the picker


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert re.search(r"_ZN3gsr12k_attr_statsE\w+", out)
    assert len(set(re.findall(r"_ZN3gsr11k_attr_histILi[01]EEEv\w*", out))) == 2      # the peel and the plain form
    assert re.search(r"_ZN3gsr13k_attr_selectE\w+", out)
    assert re.search(r"_ZN3gsr16k_contrib_selectE\w+", out)


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--histogram ATTR[:BINS]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_attr_stats", "gsr_attr_histogram", "gsr_select_attr", "attr_stats_ms", "attr_histogram_ms", "select_attr_ms", "histogram_equals_selection"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_attr_histogram", "attr_histogram", "splatHistogram", "select_attr", "selectAttribute")),
                        ("DESIGN.md", ("\"Splat data\"", "k_attr_stats", "k_attr_hist", "k_attr_select", "5.15", "8.i", "attribute pickers"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
