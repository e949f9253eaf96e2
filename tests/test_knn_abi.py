"""k nearest neighbours, the part that needs no GPU: the two entry points are exported by the library, prototyped by the Python
host and documented in include/gsplat_hip.h, the way tests/test_neighbour_abi.py holds neighbours to the header; the sources are
wired into every build, the kernels are in the code object by name, the host file compiles clean under -Wall -Wextra, and the C++
caller lists its option."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_knn", "gsr_select_knn")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info = ctypes.POINTER(gh.GsrKnnInfo)
    assert lib.gsr_knn.argtypes == [vp, f64, u32, u32, u64, i32, vp, vp, vp, vp, u32, vp, info]
    assert lib.gsr_select_knn.argtypes == [vp, f64, u32, u32, u64, i32, f64, f64, i32, ctypes.POINTER(u32), info]
    K = gh.GsrKnnInfo
    assert ctypes.sizeof(K) == 48
    assert [(f[0], getattr(K, f[0]).offset) for f in K._fields_] == [("in_scope", 0), ("nonfinite", 4), ("pair_bound", 8), ("budget", 16), ("complete", 24),
                                                                    ("finite_values", 28), ("value_min", 32), ("value_max", 40)]
    # NULL ctx: refused without a device
    assert lib.gsr_knn(None, 1.0, 8, 0, 0, 1, None, None, None, None, 0, None, None) == -1
    assert lib.gsr_select_knn(None, 1.0, 8, 0, 0, 1, 0.0, 1.0, 0, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_KNN_MAX_K 32u", "#define GSR_KNN_NONE 0xffffffffu", "#define GSR_KNN_KTH 0", "#define GSR_KNN_MEAN 1",
                 "typedef struct gsr_knn_info { uint32_t in_scope; uint32_t nonfinite; uint64_t pair_bound; uint64_t budget; uint32_t complete; uint32_t finite_values; "
                 "double value_min; double value_max; } gsr_knn_info;",
                 "int gsr_knn(gsr_ctx *ctx, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat, uint32_t *found, uint32_t *idx, double *d2, "
                 "double *values, uint32_t n, uint32_t *hist, gsr_knn_info *info);",
                 "int gsr_select_knn(gsr_ctx *ctx, double radius, uint32_t k, uint32_t scope, uint64_t budget, int32_t stat, double lo, double hi, int32_t op, "
                 "uint32_t *selected, gsr_knn_info *info);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- k nearest neighbours ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on k nearest neighbours"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definition, the two calls, the consistency guarantee, the budget, state and ordering, the refusals, the scratch
    for words in ("exactly those of \"neighbours\"", "a distance of exactly radius counts", "nobody's neighbour", "the k nearest WITHIN radius", "1 <= k <= GSR_KNN_MAX_K",
                  "ordered ascending by the pair (d2(i,j), j)", "equal distances go to the smaller index", "m_i = min(k, |N_i|)", "GSR_KNN_NONE and +inf for m_i <= t < k",
                  "m_i == k ? sqrt(dd_i[k-1]) : +inf", "sqrt correctly rounded", "m_i == 0 ? +inf", "summed in ascending t, uncontracted", "value_i = NaN (0x7ff8000000000000) for i not in S",
                  "A non-finite splat in S has m_i = 0 and value +inf", "do not depend on any visiting order", "any out pointer may be NULL", "row i of a list at [i * k]",
                  "a non-NULL per-splat pointer with n not equal to the scene's count is refused", "Rows outside S hold found = 0, GSR_KNN_NONE, +inf and NaN",
                  "sum(hist) == info->in_scope", "info may be NULL", "An empty scene, or an empty scope, returns zeros", "complete = the splats with m_i == k",
                  "+inf / -inf when there is none", "every field is exact", "lo <= value_i && (value_i < hi || hi == +inf)", "hi = +inf means \"no upper end\"",
                  "the one difference from gsr_select_attr", "lo == hi (both finite) picks nothing", "statistical outlier removal", "gsr_scene_erase_selected",
                  "The consistency guarantee", "The work budget is the neighbour budget", "launches no walk", "one 27-cell walk", "blocking and stateless",
                  "nothing can go stale after an edit", "ordered like gsr_select_attr", "wait for every member's stream", "write none of it", "a NULL ctx",
                  "k outside 1 .. 32", "unknown scope flags, stat or op", "a NaN bound or lo > hi", "a wrong n", "the selection and its count included",
                  "belongs to the context", "4 + 8 bytes per splat for found and values", "12 bytes per splat per k for the lists, only when idx or d2 is asked for",
                  "The first call allocates it, it only grows", "gsr_destroy frees it", "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("knn", "select_knn", "select_statistical_outliers"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("splatKnn(", "selectKnn(", "selectStatisticalOutliers("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_knn.hip" in srcs and "gsr_knn.cpp" in srcs                  # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(CSRC, "k_knn.hip")).read()
    assert "GSR_BOUNDS_DECL(knn)" in src and '#include "k_neighbours.h"' in src
    for site in range(8):                                                 # set word, entry slot, bucket, LDS list slot, LDS counter, global counter, selection word, splat row
        assert re.search(r"GSR_BOUND\(knn, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                              # plain HIP: ordinary vector stores and HIP atomics only
    for word in ("nb_each_cell<knn_sites>(", "nb_grid(", "__hip_atomic_fetch_add", "__hip_atomic_fetch_max", "__HIP_MEMORY_SCOPE_AGENT", "__HIP_MEMORY_SCOPE_WORKGROUP", "__ATOMIC_RELAXED",
                 "__ballot", "__shfl_xor", "extern __shared__", "__dsqrt_rn(", "!(d <= ix.r2)"):
        assert word in code, word
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)\b\*", code)       # integer atomics only
    host = open(os.path.join(CSRC, "gsr_knn.cpp")).read()
    for word in ("settle_members(c)", "select_ensure(c)", "select_fold_and_count(c, op, selected)", "nb_check(c, who, radius, k, scope, budget, 1u, \"k\", GSR_KNN_MAX_K)",
                 "nb_index(c, who, radius, k, scope, budget, true", "GSR_NEIGHBOUR_DEFAULT_BUDGET"):
        assert word in host, word
    api = open(os.path.join(CSRC, "gsr_api.cpp")).read()
    assert "c->knn.ev" in api                                             # gsr_destroy lets go of it


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr5k_knnILi[01]ELb[01]EEEv\w*?Pj\b", out))) == 4  # kth and mean, with and without the lists
    assert re.search(r"_ZN3gsr10k_knn_fillE\w+", out)
    assert re.search(r"_ZN3gsr12k_knn_selectE\w+", out)


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_knn.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_knn.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--knn RADIUS:K[:kth|mean]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_knn(", "gsr_select_knn(", "index_build_ms", "walk_ms", "lists_walk_ms", "pair_bound", "pair_tests_per_s", "values_equal_selection"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_knn", "gsr_select_knn", "splatKnn", "selectKnn", "selectStatisticalOutliers", "select_statistical_outliers",
                                       "--knn RADIUS:K[:kth|mean]")),
                        ("DESIGN.md", ("\"k nearest neighbours\"", "k_knn", "k_knn_fill", "k_knn_select", "5.18", "8.l", "pair_bound", "GSR_KNN_MAX_K",
                                       "GSR_NEIGHBOUR_DEFAULT_BUDGET"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
