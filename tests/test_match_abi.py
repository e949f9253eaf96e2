"""Matching and registration, the part that needs no GPU: the six entry points are exported by the library, prototyped by the Python
host and documented in include/gsplat_hip.h, the way tests/test_plane_abi.py holds planes to the header; the sources are wired into
every build, the kernels are in the code object by name, the host file compiles clean under -Wall -Wextra, the pure functions run
without a device and equal the reference bit for bit, and the C++ caller lists its option."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import register_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_match", "gsr_select_match", "gsr_register", "gsr_rigid_solve", "gsr_rigid_compose", "gsr_rigid_decompose")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info, sums, reg = ctypes.POINTER(gh.GsrMatchInfo), ctypes.POINTER(gh.GsrMatchSums), ctypes.POINTER(gh.GsrRegisterInfo)
    assert lib.gsr_match.argtypes == [vp, vp, vp, f64, u32, u32, u64, vp, vp, u32, sums, info]
    assert lib.gsr_select_match.argtypes == [vp, vp, vp, f64, u32, u32, u64, f64, f64, i32, ctypes.POINTER(u32), info]
    assert lib.gsr_register.argtypes == [vp, vp, vp, f64, u32, u32, u64, u32, f64, vp, reg]
    assert lib.gsr_rigid_solve.argtypes == [sums, vp, ctypes.POINTER(f64)]
    assert lib.gsr_rigid_compose.argtypes == [vp, vp, vp] and lib.gsr_rigid_decompose.argtypes == [vp, vp, vp]
    I, S, R = gh.GsrMatchInfo, gh.GsrMatchSums, gh.GsrRegisterInfo
    assert ctypes.sizeof(I) == 48 and ctypes.sizeof(S) == 136 and ctypes.sizeof(R) == 56
    assert [f[0] for f in I._fields_] == ["in_scope", "nonfinite", "target_indexed", "matched", "pair_bound", "budget", "d2_min", "d2_max"]
    assert (I.target_indexed.offset, I.pair_bound.offset, I.budget.offset, I.d2_min.offset, I.d2_max.offset) == (8, 16, 24, 32, 40)
    assert (S.pairs.offset, S.sum.offset) == (0, 8)
    assert [f[0] for f in R._fields_] == ["status", "iterations", "pairs", "rms", "delta", "step_pairs", "step_rms", "step_rows", "reserved"]
    assert (R.pairs.offset, R.rms.offset, R.delta.offset, R.step_pairs.offset, R.step_rms.offset, R.step_rows.offset) == (8, 16, 24, 32, 40, 48)
    # NULL ctx: refused without a device
    assert lib.gsr_match(None, None, None, 0.1, 0, 0, 0, None, None, 0, None, None) == -1
    assert lib.gsr_select_match(None, None, None, 0.1, 0, 0, 0, 0.0, 1.0, 0, None, None) == -1
    assert lib.gsr_register(None, None, None, 0.1, 0, 0, 0, 4, 0.0, None, None) == -1
    assert lib.gsr_rigid_solve(None, None, None) == -1 and lib.gsr_rigid_compose(None, None, None) == -1 and lib.gsr_rigid_decompose(None, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_MATCH_NONE 0xffffffffu", "#define GSR_REGISTER_CONVERGED 0", "#define GSR_REGISTER_MAX_ITERATIONS 1", "#define GSR_REGISTER_TOO_FEW 2",
                 "#define GSR_REGISTER_MAX_ITERATIONS_LIMIT 256u",
                 "typedef struct gsr_match_info { uint32_t in_scope; uint32_t nonfinite; uint32_t target_indexed; uint32_t matched; uint64_t pair_bound; uint64_t budget; "
                 "double d2_min; double d2_max; } gsr_match_info;",
                 "typedef struct gsr_match_sums { uint64_t pairs; double sum[16]; } gsr_match_sums;",
                 "typedef struct gsr_register_info { int32_t status; uint32_t iterations; uint64_t pairs; double rms, delta; uint64_t *step_pairs; double *step_rms; "
                 "uint32_t step_rows; uint32_t reserved; } gsr_register_info;",
                 "int gsr_match(gsr_ctx *ctx, gsr_ctx *target, const double *M , double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, uint32_t *idx, double *d2, "
                 "uint32_t n, gsr_match_sums *sums, gsr_match_info *info);",
                 "int gsr_select_match(gsr_ctx *ctx, gsr_ctx *target, const double *M, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, double lo, double hi, "
                 "int32_t op, uint32_t *selected, gsr_match_info *info);",
                 "int gsr_register(gsr_ctx *ctx, gsr_ctx *target, const double *M0, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, uint32_t max_iterations, "
                 "double tolerance, double *M_out , gsr_register_info *info);",
                 "int gsr_rigid_solve(const gsr_match_sums *sums, double *D , double *rms);", "int gsr_rigid_compose(const double *D, const double *M, double *out );",
                 "int gsr_rigid_decompose(const double *M, double *q_xyzw, double *t );"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- matching and registration ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on matching and registration"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definitions, the calls, the solve's written order, the loop, the budget, state and ordering, the refusals, the scratch
    for words in ("All arithmetic is f64, in the written order, uncontracted", "correctly rounded", "row-major 3 x 4 (R | t)", "NULL is the identity",
                  "T_k = ((M[k][0]*p_x + M[k][1]*p_y) + M[k][2]*p_z) + M[k][3]", "S is evaluated on ctx's selection and hidden set, S' on target's",
                  "indexed iff it is in S' and its position is finite", "all three T_k are finite", "d2(i,j) = (ex*ex + ey*ey) + ez*ez", "d2 <= radius*radius",
                  "equal distances go to the smaller target index", "GSR_MATCH_NONE and +inf", "GSR_MATCH_NONE and NaN", "gsr_knn's convention",
                  "There is no \"other\" exclusion", "the smallest index among the splats coincident with it", "h = radius * (1 + 2^-10)", "floor(T_k * inv_h)",
                  "T_a*Q_b for ab = 00, 01, 02, 10, 11, 12, 20, 21, 22, d2", "sixteen +0.0", "groups of 256 consecutive rows", "padded with +0.0",
                  "for s = 128, 64, .., 1: x[l] = x[l] + x[l + s] for l < s", "the tree decides the bits", "pairs is the integer count of matched splats",
                  "the tree runs only when sums are asked for", "d2_min +inf, d2_max -inf", "lo <= v_i && (v_i < hi || hi == +inf)", "v_i = sqrt(d2_i)",
                  "\"what it lacks\"", "The consistency guarantee", "Horn's closed form", "inv = 1.0 / n", "S_ab = sum[6 + 3*a + b] * inv - mT_a * mQ_b",
                  "N00 = (Sxx + Syy) + Szz", "N01 = Syz - Szy", "N02 = Szx - Sxz", "N03 = Sxy - Syx", "N11 = (Sxx - Syy) - Szz", "N12 = Sxy + Syx", "N13 = Szx + Sxz",
                  "N22 = (Syy - Sxx) - Szz", "N23 = Syz + Szy", "N33 = (Szz - Sxx) - Syy", "exactly 8 sweeps", "(0,1), (0,2), (0,3), (1,2), (1,3), (2,3)",
                  "\"merging cells\", step 6", "th = (A_qq - A_pp) / (2.0 * A_pq)", "for both r other than p, q", "ties to the smallest k",
                  "sqrt(((w*w + x*x) + y*y) + z*z)", "negated if its first non-zero component is negative", "R00 = 1.0 - 2.0*(y*y + z*z)", "R21 = 2.0*(y*z + x*w)",
                  "t_k = mQ_k - ((R_k0*mT_0 + R_k1*mT_1) + R_k2*mT_2)", "rms = sqrt(sum[15] * inv)", "pairs < 3, a non-finite sum", "is not detected",
                  "tests/register_reference.py", "out = D o M (apply M, then D)", "plus D[k][3] for c == 3", "Shepperd's four branches", "step 9",
                  "gsr_scene_rotate(q) then gsr_scene_translate(t)", "GSR_REGISTER_TOO_FEW", "M_{t+1} = D_t o M_t", "<= tolerance", "GSR_REGISTER_CONVERGED",
                  "GSR_REGISTER_MAX_ITERATIONS", "All three return GSR_OK", "step_rows >= max_iterations", "The scene is never written", "do not drift",
                  "its index is built once per call", "Rigid only", "The work budget is the neighbour budget", "populations of the 27 buckets their walk visits",
                  "at every step of gsr_register", "naming both numbers", "launches no walk", "blocking and stateless", "both contexts' shared scenes",
                  "target must be on ctx's device", "target's scene, selection, hidden set and frame state are not changed", "a NULL ctx or target", "another device",
                  "the radius rules of \"neighbours\"", "unknown scope flags or op", "a NaN bound or lo > hi", "a wrong n", "a non-finite M",
                  "a tolerance that is NaN or negative", "iterations outside 1 .. 256", "a budget above the maximum", "a bound above the budget",
                  "the selection and its count included", "sized for the TARGET's count", "4 + 8 bytes per source splat", "the tree's partial rows",
                  "The first call allocates it, it only grows", "gsr_destroy frees it", "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("match", "select_match", "register"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    for name in ("rigid_solve", "rigid_compose", "rigid_decompose"):
        assert callable(getattr(gh, name)), name
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("matchScene(", "selectMatch(", "registerTo(", "rigidDecompose("):
        assert name in dts, name


def test_pure_functions_need_no_device_and_equal_the_reference():
    import gsplat_hip as gh
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)
    src, tgt, _ = rr.scenario(False)
    M = rr.IDENTITY.copy()
    for step in range(3):
        idx, d2, _ = rr.match(src, tgt, rr.RADIUS, M)
        pairs, s16 = rr.sums(src, tgt, idx, d2, M)
        D, rms = rr.rigid_solve(pairs, s16)
        gD, grms = gh.rigid_solve({"pairs": pairs, "sum": s16})
        assert np.array_equal(bits(gD), bits(D)) and bits([grms])[0] == bits([rms])[0], step
        M2 = rr.rigid_compose(D, M)
        assert np.array_equal(bits(gh.rigid_compose(D, M)), bits(M2)), step
        q, t = rr.rigid_decompose(M2)
        gq, gt = gh.rigid_decompose(M2)
        assert np.array_equal(bits(gq), bits(q)) and np.array_equal(bits(gt), bits(t)), step
        M = M2
    with pytest.raises(gh.GsplatError) as ei:
        gh.rigid_solve({"pairs": 2, "sum": np.zeros(16)})
    assert ei.value.code == -1 and "at least 3" in str(ei.value)
    with pytest.raises(gh.GsplatError):
        gh.rigid_decompose(np.full(12, np.nan))


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_match.hip" in srcs and "gsr_match.cpp" in srcs           # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(CSRC, "k_match.hip")).read()
    assert "GSR_BOUNDS_DECL(match)" in src and "struct match_sites" in src
    for site in range(8):                                              # set word, source row, bucket, entry slot, target row, partial row, selection word, LDS cell
        assert re.search(r"GSR_BOUND\(match, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                           # plain C++ and HIP atomics only
    for word in ("__hip_atomic_fetch_add", "__hip_atomic_fetch_max", "__HIP_MEMORY_SCOPE_AGENT", "__ATOMIC_RELAXED", "__ballot", "__shfl_down(", "__shfl_xor(",
                 "in_scope<match_sites>(", "mask_store_ballot<match_sites>(", "workgroup_sum_u64<NB_THREADS>(", "nb_each_near_query<match_sites>(",
                 "nb_each_cell<match_sites>(", "nb_cell_query(", "__dsqrt_rn(", "__shared__ double s_rows[MATCH_ROW * MATCH_GROUP]", "f32_finite("):
        assert word in code, word
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)", code)   # integer atomics only
    assert "fma(" not in code
    walk = code[code.index("void k_match("):code.index("__device__ __forceinline__ void tree_reduce(")]
    assert "__shared__" not in walk and walk.count("__hip_atomic_fetch") == 3                    # no LDS; matched, max and min once per wave
    shared = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_neighbours.h")).read())
    for word in ("nb_cell_query(double v, double inv_h)", "void nb_each_near_query(", "constexpr uint32_t NB_QUERY_BATCH = 4;", "ck[u] != nk"):
        assert word in shared, word
    query = shared[shared.index("void nb_each_near_query("):]
    assert query.index("ck[u] != nk") < query.index("ex * ex")        # the key is compared before any f64
    assert "holds unchanged for a query point given as a double" in open(os.path.join(CSRC, "k_neighbours.hip")).read()
    host = open(os.path.join(CSRC, "gsr_match.cpp")).read()
    for word in ("settle_members(c)", "select_ensure(c)", "select_fold_and_count(c, op, selected)", "GSR_NEIGHBOUR_DEFAULT_BUDGET", "scope_check(c, who, target_scope)",
                 "nb_check(c, who, radius, 1u, scope, budget)", "nb_prepare_rows(c, who, tn ? tn : 1u,", "gsr_debug_match_times", "gsr_debug_match_scratch"):
        assert word in host, word
    ctx = open(os.path.join(CSRC, "gsr_api.cpp")).read()
    assert "c->mt.ev" in ctx                                           # the events go with the context


def test_the_constants_of_the_tests_are_the_source():
    internal = open(os.path.join(CSRC, "gsr_internal.h")).read()
    assert int(re.search(r"constexpr uint32_t MATCH_GROUP = (\d+);", internal).group(1)) == rr.GROUP
    assert int(re.search(r"constexpr uint32_t MATCH_ROW = (\d+);", internal).group(1)) == 16
    header = open(HEADER).read()
    assert int(re.search(r"#define GSR_REGISTER_MAX_ITERATIONS_LIMIT (\d+)u", header).group(1)) == rr.MAX_STEPS
    assert (int(re.search(r"#define GSR_REGISTER_CONVERGED\s+(\d+)", header).group(1)), int(re.search(r"#define GSR_REGISTER_MAX_ITERATIONS\s+(\d+)", header).group(1)),
            int(re.search(r"#define GSR_REGISTER_TOO_FEW\s+(\d+)", header).group(1))) == (rr.CONVERGED, rr.MAX_ITERATIONS, rr.TOO_FEW)
    sizes = sorted({f[1].shape[0] for f in rr.families()})
    for n in (1, 63, 64, 65, 255, 256, 257, 65536, 65537):            # wave, workgroup and tree-group edges; the tree's third level and its padding
        assert n in sizes, n
    assert max(f[1].shape[0] * f[2].shape[0] for f in rr.families()) <= 65537 * 512


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    for name in ("_ZN3gsr13k_match_boundE", "_ZN3gsr7k_matchE", "_ZN3gsr12k_match_rowsE", "_ZN3gsr12k_match_treeE", "_ZN3gsr14k_match_selectE"):
        assert re.search(name + r"\w+", out), name
    twin = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
    if os.path.exists(twin):
        t = subprocess.run(["strings", "-a", twin], capture_output=True, text=True).stdout
        assert "gsr_debug_bounds_match" in t and "gsr_debug_bounds_match" not in out


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_match.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_match.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--register RADIUS[:ITERATIONS]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_register(", "gsr_scene_rotate(tgt", "gsr_scene_translate(tgt", "gsr_debug_match_times", "register_ms", "index_build_ms", "bound_ms", "walk_ms", "tree_ms",
                 "step_pairs", "step_rms"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_match", "gsr_select_match", "gsr_register", "gsr_rigid_solve", "gsr_rigid_decompose", "matchScene", "selectMatch", "registerTo",
                                       "select_match", "rigid_decompose", "--register RADIUS[:ITERATIONS]")),
                        ("DESIGN.md", ("\"Matching and registration\"", "k_match_bound", "k_match_rows", "k_match_tree", "k_match_select", "nb_each_near_query", "5.21", "8.p",
                                       "Horn", "a similarity solve", "point-to-plane", "a source ordered by target cell", "built once per `gsr_register`",
                                       "do not drift"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
