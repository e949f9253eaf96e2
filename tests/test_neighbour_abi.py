"""Neighbours, the part that needs no GPU: the two entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_attr_abi.py holds splat data to the header; the sources are wired into
every build, the kernels are in the code object by name, the host file compiles clean under -Wall -Wextra, and the C++ caller lists
its option."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_neighbours", "gsr_select_neighbours")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info = ctypes.POINTER(gh.GsrNeighbourInfo)
    assert lib.gsr_neighbours.argtypes == [vp, f64, u32, u32, u64, vp, u32, vp, info]
    assert lib.gsr_select_neighbours.argtypes == [vp, f64, u32, u32, u64, u32, u32, i32, ctypes.POINTER(u32), info]
    assert ctypes.sizeof(gh.GsrNeighbourInfo) == 24 and gh.GsrNeighbourInfo.pair_bound.offset == 8 and gh.GsrNeighbourInfo.budget.offset == 16
    # NULL ctx: refused without a device
    assert lib.gsr_neighbours(None, 1.0, 8, 0, 0, None, 0, None, None) == -1
    assert lib.gsr_select_neighbours(None, 1.0, 8, 0, 0, 0, 1, 0, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_NEIGHBOUR_MAX_CAP 4095u", "#define GSR_NEIGHBOUR_DEFAULT_BUDGET (1ull << 34)", "#define GSR_NEIGHBOUR_MAX_BUDGET (1ull << 38)",
                 "typedef struct gsr_neighbour_info { uint32_t in_scope; uint32_t nonfinite; uint64_t pair_bound; uint64_t budget; } gsr_neighbour_info;",
                 "int gsr_neighbours(gsr_ctx *ctx, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t *counts, uint32_t n, uint32_t *hist, gsr_neighbour_info *info);",
                 "int gsr_select_neighbours(gsr_ctx *ctx, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t lo, uint32_t hi, int32_t op, uint32_t *selected, gsr_neighbour_info *info);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- neighbours ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on neighbours"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definition, the two calls, the consistency guarantee, the budget, state and ordering, the refusals, the scratch
    for words in ("dx = (double)x_i - (double)x_j", "d2(i,j) = (dx*dx + dy*dy) + dz*dz", "r2 = radius * radius", "near(i,j) := i != j && d2(i,j) <= r2",
                  "count_i = min(cap, #{ j in S : near(i,j) })", "count_i = 0 for i not in S", "d2 is symmetric", "Distance exactly radius counts",
                  "Coincident splats count each other", "A splat does not count itself", "nobody's neighbour", "kept out of the index",
                  "independent of the order of arrival", "GSR_SCOPE_SELECTED | GSR_SCOPE_VISIBLE", "0 is every splat",
                  "a non-NULL counts with n not equal to the scene's count is refused", "hist[cap] means \"cap or more\"", "sum(hist) == info->in_scope",
                  "info may be NULL", "An empty scene, or an empty scope, returns zeros", "lo <= count_i && count_i < hi", "lo <= hi <= cap + 1",
                  "lo == hi picks nothing", "The consistency guarantee", "exactly sum(hist[lo .. hi-1]) splats", "radius outlier removal",
                  "gsr_scene_erase_selected", "The work budget", "O(n^2)", "pair_bound > budget", "naming both numbers", "launches no count kernel",
                  "budget == 0 means GSR_NEIGHBOUR_DEFAULT_BUDGET", "above GSR_NEIGHBOUR_MAX_BUDGET is refused", "never below the exact 27-cell neighbourhood sum",
                  "blocking and stateless", "nothing can go stale after an edit", "ordered like gsr_select_attr", "wait for every member's stream",
                  "write none of it", "no frame state changes", "a NULL ctx", "not finite, not > 0", "radius * radius or 1 / radius not finite and normal",
                  "cap outside 1 .. 4095", "unknown scope flags or op", "lo > hi or hi > cap + 1", "the selection and its count included",
                  "belongs to the context", "The first call allocates it, it only grows", "gsr_destroy frees it", "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("neighbours", "select_neighbours"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("splatNeighbours(", "selectNeighbours("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_neighbours.hip" in srcs and "gsr_neighbours.cpp" in srcs    # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(CSRC, "k_neighbours.hip")).read()
    assert "GSR_BOUNDS_DECL(neighbours)" in src
    for site in range(8):                                                 # set word, splat index, bucket, entry slot, LDS counter, global counter, selection word, counts word
        assert re.search(r"GSR_BOUND\(neighbours, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                              # ordinary vector stores and HIP atomics only
    for word in ("__hip_atomic_fetch_add", "__HIP_MEMORY_SCOPE_AGENT", "__HIP_MEMORY_SCOPE_WORKGROUP", "__ATOMIC_RELAXED", "__ballot", "in_scope<nb_sites>(", "extern __shared__",
                 "floor("):
        assert word in code, word
    ops = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_splat_ops.h")).read())
    assert "set_word(" in ops[ops.index("uint32_t scope_word("):ops.index("bool in_scope(")]       # the scope reads the sets through set_word, for every unit
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)", code)      # integer atomics only
    assert "trunc" not in code                                            # floor, not truncation
    host = open(os.path.join(CSRC, "gsr_neighbours.cpp")).read()
    for word in ("settle_members(c)", "select_ensure(c)", "select_fold_and_count(c, op, selected)", "GSR_NEIGHBOUR_DEFAULT_BUDGET", "scope_check(c, who, scope, budget)"):
        assert word in host, word
    assert "GSR_NEIGHBOUR_MAX_BUDGET" in open(os.path.join(CSRC, "gsr_attr.cpp")).read()           # scope_check's refusal, shared with gsr_merge.cpp


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr10k_nb_cellsILb[01]EEEv\w*", out))) == 2       # the count and the scatter
    assert re.search(r"_ZN3gsr12k_nb_offsetsE\w+", out)
    assert re.search(r"_ZN3gsr10k_nb_boundE\w+", out)
    assert len(set(re.findall(r"_ZN3gsr10k_nb_countILb[01]EEEv\w*", out))) == 2       # with and without the histogram
    assert re.search(r"_ZN3gsr11k_nb_selectE\w+", out)


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_neighbours.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_neighbours.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--neighbours RADIUS[:CAP]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_neighbours", "gsr_select_neighbours", "index_build_ms", "count_ms", "pair_bound", "pair_tests_per_s", "histogram_equals_selection"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_neighbours", "gsr_select_neighbours", "splatNeighbours", "selectNeighbours", "select_neighbours", "--neighbours RADIUS[:CAP]")),
                        ("DESIGN.md", ("\"Neighbours\"", "k_nb_cells", "k_nb_offsets", "k_nb_bound", "k_nb_count", "k_nb_select", "5.16", "8.j", "pair_bound",
                                       "GSR_NEIGHBOUR_DEFAULT_BUDGET"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
