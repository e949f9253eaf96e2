"""Clusters, the part that needs no GPU: the three entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_neighbour_abi.py holds neighbours to the header; the sources are wired into
every build, the index's walk is stated once for both users, the kernels are in the code object by name, the host file compiles
clean under -Wall -Wextra, and the C++ caller lists its option."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_clusters", "gsr_select_clusters", "gsr_select_cluster_at")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info = ctypes.POINTER(gh.GsrClusterInfo)
    assert lib.gsr_clusters.argtypes == [vp, f64, u32, u32, u64, vp, vp, u32, info]
    assert lib.gsr_select_clusters.argtypes == [vp, f64, u32, u32, u64, u32, u32, i32, ctypes.POINTER(u32), info]
    assert lib.gsr_select_cluster_at.argtypes == [vp, f64, u32, u32, u64, u32, i32, ctypes.POINTER(u32), info]
    I = gh.GsrClusterInfo
    assert ctypes.sizeof(I) == 48
    assert [(f[0], getattr(I, f[0]).offset) for f in I._fields_] == [("in_scope", 0), ("nonfinite", 4), ("pair_bound", 8), ("budget", 16), ("core", 24),
                                                                    ("border", 28), ("noise", 32), ("clusters", 36), ("largest_label", 40), ("largest_size", 44)]
    # NULL ctx: refused without a device
    assert lib.gsr_clusters(None, 1.0, 0, 0, 0, None, None, 0, None) == -1
    assert lib.gsr_select_clusters(None, 1.0, 0, 0, 0, 0, 1, 0, None, None) == -1
    assert lib.gsr_select_cluster_at(None, 1.0, 0, 0, 0, 0, 0, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_CLUSTER_NONE 0xffffffffu", "#define GSR_CLUSTER_LARGEST 0xffffffffu",
                 "typedef struct gsr_cluster_info { uint32_t in_scope; uint32_t nonfinite; uint64_t pair_bound; uint64_t budget; uint32_t core; uint32_t border; "
                 "uint32_t noise; uint32_t clusters; uint32_t largest_label; uint32_t largest_size; } gsr_cluster_info;",
                 "int gsr_clusters(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t *labels, uint32_t *sizes, uint32_t n, gsr_cluster_info *info);",
                 "int gsr_select_clusters(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t size_lo, uint32_t size_hi, int32_t op, "
                 "uint32_t *selected, gsr_cluster_info *info);",
                 "int gsr_select_cluster_at(gsr_ctx *ctx, double radius, uint32_t min_pts, uint32_t scope, uint64_t budget, uint32_t seed, int32_t op, uint32_t *selected, "
                 "gsr_cluster_info *info);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- clusters ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on clusters"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definition, the three calls, the consistency guarantee, the budget, state and ordering, the refusals, the scratch
    for words in ("exactly those of \"neighbours\"", "a distance of exactly radius counts", "is in scope, is never indexed and is nobody's neighbour",
                  "min_pts in 0 .. GSR_NEIGHBOUR_MAX_CAP", "deg_i = #{ j in S : near(i,j) }", "the count may stop at min_pts",
                  "core_i := i in S, finite, deg_i >= min_pts", "plain connected components", "i ~ j := core_i && core_j && near(i,j)",
                  "the classes of the transitive closure of ~ over core splats", "label_i = the smallest splat index in i's class",
                  "label_i = min{ label_j : core_j && near(i,j) }", "label_i = GSR_CLUSTER_NONE", "size_i = #{ k : label_k == label_i }",
                  "A border splat never joins two clusters", "does not depend on any visiting order", "ties going to the smallest label",
                  "every member of a shared scene", "labels and sizes are n words each, or NULL", "sizes is per splat", "info may be NULL",
                  "An empty scene, or an empty scope, returns zeros", "size_lo <= size_i && size_i < size_hi", "size_lo <= size_hi", "The consistency guarantee",
                  "removes noise and every island smaller than k", "label_i == label_seed && label_seed != GSR_CLUSTER_NONE", "GSR_CLUSTER_LARGEST for the largest cluster",
                  "picks the empty set: the fold still happens", "gsr_selection_invert", "in_scope == core + border + noise", "noise including the non-finite ones",
                  "The work budget is the neighbour budget", "checked before any walk is launched", "naming both numbers", "launches no walk",
                  "up to three 27-cell walks", "the budget bounds each walk, not their sum", "blocking and stateless", "ordered like gsr_select_attr",
                  "wait for every member's stream", "write none of it", "no frame state changes", "a NULL ctx", "min_pts above 4095", "unknown scope flags or op",
                  "size_lo > size_hi", "a seed that is neither below the scene's count nor GSR_CLUSTER_LARGEST", "a wrong n", "the selection and its count included",
                  "step limit of n", "GSR_ERR_HIP", "belongs to the context", "The first cluster call allocates it, it only grows", "gsr_destroy frees it",
                  "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("clusters", "select_clusters", "select_cluster_at"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("splatClusters(", "selectClusters(", "selectClusterAt("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_clusters.hip" in srcs and "gsr_clusters.cpp" in srcs        # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id and "k_neighbours.h" in build_id
    assert "k_neighbours.h" in re.search(r"^\$\(OUT\)/%\.o: %\.hip (.*)$", mk, flags=re.M).group(1)
    files = {f: open(os.path.join(CSRC, f)).read() for f in ("k_clusters.hip", "k_neighbours.hip", "k_neighbours.h")}
    # the key, the bucket and the 27-cell walk are stated once, for both users
    for f in ("k_clusters.hip", "k_neighbours.hip"):
        assert '#include "k_neighbours.h"' in files[f], f
        for helper in ("nb_key(", "nb_bucket(", "nb_each_cell(", "nb_each_near("):
            assert not re.search(r"__device__[^;{]*\b" + re.escape(helper), files[f]), (f, helper)
    for helper in ("nb_key(", "nb_bucket(", "nb_each_cell(", "nb_each_near("):
        assert re.search(r"__device__[^;{]*\b" + re.escape(helper), files["k_neighbours.h"]), helper
    src = files["k_clusters.hip"]
    assert "GSR_BOUNDS_DECL(clusters)" in src
    for site in range(8):                                                 # set word, entry slot, bucket, parent / label word, size word, selection word, counts word, sizes word
        assert re.search(r"GSR_BOUND\(clusters, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                              # ordinary vector stores and HIP atomics only
    for word in ("atomicCAS(&parent[big], big, small)", "__hip_atomic_load", "__hip_atomic_fetch_max", "__hip_atomic_fetch_add", "__HIP_MEMORY_SCOPE_AGENT",
                 "__ATOMIC_RELAXED", "__ballot", "nb_each_near<cl_sites>(", "cl_fault("):
        assert word in code, word
    near = re.sub(r"//.*", "", files["k_neighbours.h"])
    assert "nb_each_cell<Sites>(" in near[near.index("void nb_each_near("):]     # the near walk is the 27-cell walk
    assert code.count("atomicCAS(") == 1                                  # a hook is ONE compare-and-swap
    assert not re.search(r"while\s*\(\s*(true|1)\s*\)", code) and "__builtin_amdgcn_s_sleep" not in code     # no lane waits for another
    assert not re.search(r"atomic\w*\([^;]*(float|double)", code)         # integer atomics only
    head = src[:src.index("#include")]
    for words in ("INVARIANT: parent[x] <= x at every instant", "TERMINATION", "strictly smaller index", "No lane ever waits for another lane", "step limit of n",
                  "GSR_ERR_HIP"):
        assert words in head, words
    host = open(os.path.join(CSRC, "gsr_clusters.cpp")).read()
    for word in ("settle_members(c)", "select_ensure(c)", "select_fold_and_count(c, op, selected)", "nb_index(", "nb_check(", "GSR_NEIGHBOUR_DEFAULT_BUDGET",
                 "got.fault"):
        assert word in host, word
    ctx = open(os.path.join(CSRC, "gsr_ctx.h")).read()
    assert re.search(r"^int nb_index\(", ctx, flags=re.M) and re.search(r"^int nb_check\(", ctx, flags=re.M)   # the index's host side, shared through the header


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    for name in ("9k_cl_seed", "10k_cl_union", "12k_cl_flatten", "11k_cl_border", "10k_cl_sizes", "17k_cl_select_sizes", "17k_cl_select_label"):
        assert re.search(r"_ZN3gsr%sE\w+" % name, out), name


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_clusters.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_clusters.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--clusters RADIUS[:MIN_PTS]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_clusters", "gsr_select_clusters", "index_ms", "core_ms", "union_ms", "border_ms", "largest_size", "noise", "sizes_equal_selection"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_clusters", "gsr_select_clusters", "gsr_select_cluster_at", "splatClusters", "selectClusters", "selectClusterAt",
                                       "select_clusters", "select_cluster_at", "--clusters RADIUS[:MIN_PTS]")),
                        ("DESIGN.md", ("\"Clusters\"", "k_cl_seed", "k_cl_union", "k_cl_flatten", "k_cl_border", "k_cl_sizes", "k_cl_select_sizes", "k_cl_select_label",
                                       "5.17", "8.k", "parent[x] <= x", "k_neighbours.h"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
