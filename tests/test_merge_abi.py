"""Merging cells, the part that needs no GPU: the two entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_knn_abi.py holds k nearest neighbours to the header; the sources are wired
into every build, the kernels are in the code object by name, the host file compiles clean under -Wall -Wextra, the packed
covariance is still stated once, and the C++ caller lists its option."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_cells", "gsr_scene_merge_cells")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, u32, u64, f64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info = ctypes.POINTER(gh.GsrCellInfo)
    assert lib.gsr_cells.argtypes == [vp, f64, u32, u32, u64, vp, u32, vp, info]
    assert lib.gsr_scene_merge_cells.argtypes == [vp, f64, u32, u64, ctypes.POINTER(u32), info]
    K = gh.GsrCellInfo
    assert ctypes.sizeof(K) == 48
    assert [(f[0], getattr(K, f[0]).offset) for f in K._fields_] == [("in_scope", 0), ("candidates", 4), ("cells", 8), ("merged_cells", 12), ("merged_members", 16),
                                                                    ("largest", 20), ("rows_after", 24), ("pad", 28), ("pair_bound", 32), ("budget", 40)]
    # NULL ctx: refused without a device
    assert lib.gsr_cells(None, 1.0, 8, 0, 0, None, 0, None, None) == -1
    assert lib.gsr_scene_merge_cells(None, 1.0, 0, 0, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_CELL_NONE 0xffffffffu",
                 "typedef struct gsr_cell_info { uint32_t in_scope, candidates; uint32_t cells, merged_cells; uint32_t merged_members, largest; uint32_t rows_after, pad; "
                 "uint64_t pair_bound, budget; } gsr_cell_info;",
                 "int gsr_cells(gsr_ctx *ctx, double cell, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t *leader , uint32_t n, uint32_t *hist , gsr_cell_info *info);",
                 "int gsr_scene_merge_cells(gsr_ctx *ctx, double cell, uint32_t scope, uint64_t budget, uint32_t *new_count, gsr_cell_info *info);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- merging cells ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on merging cells"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definition, the report, the merged row step by step, state and ordering, the budget, the refusals, the scratch
    for words in ("all ten floats (position, rotation, scale) are finite", "inv = 1.0 / cell, computed once on the host", "clamped to [-2^20, 2^20)", "no slack",
                  "shares the boundary cell", "the leader is the smallest member index", "GSR_CELL_NONE otherwise", "hist[cap] means \"cap or more\"", "hist[0] is 0",
                  "cap in 1 .. 4095", "rows_after = n - merged_members + merged_cells", "is left bit for bit", "written at its leader's index",
                  "order-preserving compaction gsr_scene_erase_selected uses", "*new_count == info->rows_after", "f64, uncontracted", "ascending index order",
                  "correctly rounded", "v_i = (fabs(sx) * fabs(sy)) * fabs(sz)", "If M > 0: w_i = m_i, W = M", "w_i = 1, W = (double)m", "(float)mu_k",
                  "before the factor 4 and the halves", "mu unrounded", "exactly 6 sweeps over the pairs (p, q) = (0,1), (0,2), (1,2)", "A pair with A_pq == 0 is skipped",
                  "th = (A_qq - A_pp) / (2.0 * A_pq)", "t = 1.0 / (fabs(th) + sqrt(th * th + 1.0))", "cs = 1.0 / sqrt(t * t + 1.0)", "A_rp = cs * arp - sn * arq",
                  "V_kq = sn * vkp + cs * vkq", "not sorted", "(float)sqrt(lam_k > 0 ? lam_k : 0.0)", "R = V^T: row k is eigenvector k", "Shepperd's four branches",
                  "s = sqrt(tr + 1.0) * 2.0", "x = (R21 - R12) / s, y = (R02 - R20) / s, z = (R10 - R01) / s", "((float)(-w), (float)x, (float)y, (float)z)",
                  "floor((sum w_i * c_i) / W + 0.5)", "conserves opacity x volume", "255 if o >= 255, else floor(o + 0.5)", "the largest a_i", "Data word 3 stays the leader's",
                  "blocking scene replacement", "waits for every member", "moves the generation and re-plans the bins", "the capacity is kept",
                  "a merged row has its leader's bit", "exactly as a removing erase treats them", "the selection becomes exactly the merged rows",
                  "new_count = n and changes nothing", "ordered like gsr_neighbours", "population of the candidate's own hash bucket", "GSR_NEIGHBOUR_DEFAULT_BUDGET",
                  "launches no walk", "a NULL ctx", "1 / cell not finite and normal", "cap outside 1 .. 4095", "unknown scope flags", "a non-NULL leader with the wrong n",
                  "a scene without rotations / scales", "a scene with SH rows (sh_count != 0)", "gsr_cells answers for such a scene", "belongs to the context",
                  "The first call allocates it, it only grows", "gsr_destroy frees it", "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("cells", "scene_merge_cells"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("splatCells(", "mergeCells("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_merge.hip" in srcs and "gsr_merge.cpp" in srcs              # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    assert "FLAGS_k_merge" not in mk and "FLAGS_gsr_merge" not in mk       # the flags that apply to every device file, no others
    src = open(os.path.join(CSRC, "k_merge.hip")).read()
    assert "GSR_BOUNDS_DECL(merge)" in src and '#include "k_neighbours.h"' in src
    for site in range(8):                                                 # set word, splat index, bucket, entry slot, LDS counter, cell record, mask word, member slot
        assert re.search(r"GSR_BOUND\(merge, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                              # plain HIP: ordinary vector stores and HIP atomics only
    for word in ("nb_bucket(", "nb_grid(", "__hip_atomic_fetch_add", "__hip_atomic_fetch_max", "__HIP_MEMORY_SCOPE_AGENT", "__HIP_MEMORY_SCOPE_WORKGROUP",
                 "__ATOMIC_RELAXED", "__ballot", "__shfl_up", "extern __shared__", "__dsqrt_rn(", "splat_cov(", "pack_cov(", "floor("):
        assert word in code, word
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)\b\*", code)       # integer atomics only
    assert not re.search(r"\bdouble\s+\w+\[[a-z_]\w*\]", code)             # no f64 array sized or indexed by a variable: the state stays in registers
    cov = open(os.path.join(CSRC, "k_pack_cov.h")).read()
    assert cov.count("M[0] * M[0] + M[3] * M[3] + M[6] * M[6]") == 1 and "splat_cov(rot, scl, s);" in cov      # the six sums stated once, pack_cov on top of them
    host = open(os.path.join(CSRC, "gsr_merge.cpp")).read()
    for word in ("settle_members(c)", "require_rows(c)", "select_ensure(c)", "select_fold_and_count(c, SELOP_REPLACE, nullptr)", "scene_compact(c, ScenePred{nullptr, a.remove, 0u, a.words}",
                 "nb_prepare(c, who, cap, 1.0 / cell", "launch_nb_build(", "GSR_NEIGHBOUR_DEFAULT_BUDGET", "scope_check(c, who, scope, budget)", "sc.sh_count"):
        assert word in host, word
    assert "GSR_NEIGHBOUR_MAX_BUDGET" in open(os.path.join(CSRC, "gsr_attr.cpp")).read()           # scope_check's refusal, shared with gsr_neighbours.cpp
    scene = open(os.path.join(CSRC, "gsr_scene.cpp")).read()
    assert "also->in, also->nwords_in, also->out, also->nwords_out" in scene      # the merged rows ride the compaction the hidden set rides


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr9k_mg_walkILb[01]EEEv\w*?Pj\b", out))) == 2     # with and without the histogram
    for name in ("15k_mg_candidates", "10k_mg_bound", "12k_mg_members", "11k_mg_reduce"):
        assert re.search(r"_ZN3gsr%sE\w+" % name, out), name


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_merge.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_merge.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--merge CELL]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_cells(", "gsr_scene_merge_cells(", "merge_blocking_ms", "cells_ms", "rows_before", "rows_after", "members_per_cell", "report_equals_edit"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_cells", "gsr_scene_merge_cells", "splatCells", "mergeCells", "scene_merge_cells", "--merge CELL")),
                        ("DESIGN.md", ("\"Merging cells\"", "k_mg_candidates", "k_mg_walk", "k_mg_members", "k_mg_reduce", "5.19", "8.m", "pair_bound", "GSR_CELL_NONE",
                                       "GSR_NEIGHBOUR_DEFAULT_BUDGET"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
