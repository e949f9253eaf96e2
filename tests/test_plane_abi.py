"""Planes, the part that needs no GPU: the four entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_neighbour_abi.py holds neighbours to the header; the sources are wired into
every build, the kernels are in the code object by name, the host file compiles clean under -Wall -Wextra, the C++ caller lists its
option, and the chunk constant of the tests is the one of the source."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_fit_plane", "gsr_plane_inliers", "gsr_select_plane", "gsr_plane_alignment")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    info = ctypes.POINTER(gh.GsrPlaneInfo)
    assert lib.gsr_fit_plane.argtypes == [vp, f64, u32, u64, u32, u64, vp, info]
    assert lib.gsr_plane_inliers.argtypes == [vp, vp, u32, f64, u32, u64, vp, info]
    assert lib.gsr_select_plane.argtypes == [vp, vp, f64, f64, i32, ctypes.POINTER(u32)]
    assert lib.gsr_plane_alignment.argtypes == [vp, vp, vp, vp]
    P = gh.GsrPlaneInfo
    assert ctypes.sizeof(P) == 88 and P.tests.offset == 40 and P.budget.offset == 48 and P.plane.offset == 56
    assert [f[0] for f in P._fields_] == ["in_scope", "nonfinite", "hypotheses", "degenerate", "found", "best", "triple", "inliers", "tests", "budget", "plane"]
    assert (P.in_scope.offset, P.hypotheses.offset, P.found.offset, P.triple.offset, P.inliers.offset) == (0, 8, 16, 24, 36)
    # NULL ctx: refused without a device
    i = gh.GsrPlaneInfo()
    assert lib.gsr_fit_plane(None, 0.1, 8, 0, 0, 0, None, ctypes.byref(i)) == -1
    assert lib.gsr_plane_inliers(None, None, 1, 0.1, 0, 0, None, None) == -1
    assert lib.gsr_select_plane(None, None, 0.0, 1.0, 0, None) == -1
    assert lib.gsr_plane_alignment(None, None, None, None) == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_PLANE_MAX_HYPOTHESES 4096u",
                 "typedef struct gsr_plane_info { uint32_t in_scope, nonfinite; uint32_t hypotheses, degenerate; uint32_t found, best; uint32_t triple[3]; uint32_t inliers; "
                 "uint64_t tests, budget; double plane[4]; } gsr_plane_info;",
                 "int gsr_fit_plane(gsr_ctx *ctx, double threshold, uint32_t hypotheses, uint64_t seed, uint32_t scope, uint64_t budget, uint32_t *scores , gsr_plane_info *info);",
                 "int gsr_plane_inliers(gsr_ctx *ctx, const double *planes , uint32_t count, double threshold, uint32_t scope, uint64_t budget, uint32_t *inliers , gsr_plane_info *info);",
                 "int gsr_select_plane(gsr_ctx *ctx, const double *plane , double lo, double hi, int32_t op, uint32_t *selected);",
                 "int gsr_plane_alignment(const double *plane, const double *axis , double *q_xyzw, double *t );"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- planes ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on planes"
    doc = " ".join(re.sub(r"\n \* ?", "\n", m.group(0)).split())
    # the definitions, the four calls, the consistency guarantee, the budget, state and ordering, the refusals, the scratch
    for words in ("All arithmetic is f64, in the written order, uncontracted", "correctly rounded", "GSR_SCOPE_SELECTED | GSR_SCOPE_VISIBLE", "0 is every splat",
                  "A candidate is a splat in S whose three position floats are finite", "cand[0 .. m-1]", "nonfinite = in_scope - m",
                  "Rotation and scale are not read", "s = ((a*(double)x + b*(double)y) + c*(double)z) + d", "do not normalise them", "fabs(s) <= t",
                  "a distance of exactly t counts", "z += 0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "return z ^ (z >> 31)",
                  "rank(h, j) = mulhi64(mix(seed + 3*h + j), m)", "the high 64 bits of the 128-bit product", "A, B, C = cand[rank(h, 0..2)]", "e1 = B - A, e2 = C - A",
                  "N = (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x)", "l2 = (Nx*Nx + Ny*Ny) + Nz*Nz",
                  "degenerate if two ranks are equal, if l2 is not finite, or if l2 == 0", "n = N / sqrt(l2)",
                  "nx < 0 || (nx == 0 && (ny < 0 || (ny == 0 && nz < 0)))", "a -0.0 that this leaves behind is part of the result", "d = -((nx*Ax + ny*Ay) + nz*Az)",
                  "a degenerate hypothesis scores 0", "ties go to the smallest h", "found = 0 iff every hypothesis is degenerate", "covers m < 3",
                  "independent of the order of arrival", "scores is `hypotheses` words or NULL", "tests = hypotheses * m",
                  "An empty scene or an empty scope returns GSR_OK with zeros", "the scoring pass alone", "check a plane it refined itself", "hypotheses = count",
                  "lo <= s_i && s_i <= hi", "hidden ones included", "closed at both ends", "NaN is never picked", "\"everything under the floor\"", "NaN or lo > hi is refused",
                  "The consistency guarantee", "selects exactly info.inliers splats", "GSR_SELOP_INTERSECT", "a pure function with no context", "without a GPU",
                  "axis . p = 0", "gsr_scene_rotate(q)", "gsr_scene_translate(t)", "each normalised by their own length", "c > -1 + 2^-20", "v = n x a",
                  "q = (vx, vy, vz, 1 + c) divided by its length", "a half turn about n x e", "smallest component in magnitude", "x before y before z", "w = 0", "t = d * a",
                  "The work budget", "tests > budget", "naming both numbers", "launches no scoring kernel", "budget == 0 means GSR_NEIGHBOUR_DEFAULT_BUDGET",
                  "above GSR_NEIGHBOUR_MAX_BUDGET is refused", "blocking and stateless", "ordered like gsr_select_attr", "wait for every member's stream",
                  "write none of it", "no frame state and no selection changes", "a NULL ctx", "not finite or < 0", "hypotheses or count outside 1 .. 4096",
                  "unknown scope flags or op", "a NULL required pointer", "a non-finite entry or a zero normal", "a zero plane normal or axis",
                  "the selection and its count included", "belongs to the context", "The first call allocates it, it only grows", "gsr_destroy frees it",
                  "allocates nothing and launches nothing"):
        assert words in doc, words


def test_hosts_have_the_methods():
    import gsplat_hip as gh
    for name in ("fit_plane", "plane_inliers", "select_plane", "plane_alignment"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    assert callable(gh.plane_alignment)
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for name in ("fitPlane(", "planeInliers(", "selectPlane(", "planeAlignment("):
        assert name in dts, name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_plane.hip" in srcs and "gsr_plane.cpp" in srcs           # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the twins
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    src = open(os.path.join(CSRC, "k_plane.hip")).read()
    assert "GSR_BOUNDS_DECL(plane)" in src and "struct plane_sites" in src
    for site in range(7):                                              # set word, splat index, block-sum slot, candidate slot, hypothesis slot, selection word, LDS cell
        assert re.search(r"GSR_BOUND\(plane, %d," % site, src), site
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code                                           # plain C++ and HIP atomics only
    for word in ("__hip_atomic_fetch_add", "__HIP_MEMORY_SCOPE_AGENT", "__ATOMIC_RELAXED", "__ballot", "in_scope<plane_sites>(", "mask_store_ballot<plane_sites>(",
                 "workgroup_sum_u64<PLANE_THREADS>(", "__umul64hi(", "__dsqrt_rn(", "__shared__ double s_x[PLANE_CHUNK]", "f32_finite("):
        assert word in code, word
    assert "atomicAdd(" not in code and not re.search(r"atomic\w*\([^;]*(float|double)", code)   # integer atomics only
    assert "fma(" not in code
    score = code[code.index("void k_plane_score("):code.index("void k_plane_best(")]
    assert "__ballot" not in score and score.count("__hip_atomic_fetch_add") == 1                # no ballots, one add per lane at the end
    host = open(os.path.join(CSRC, "gsr_plane.cpp")).read()
    for word in ("settle_members(c)", "select_ensure(c)", "select_fold_and_count(c, op, selected)", "GSR_NEIGHBOUR_DEFAULT_BUDGET", "scope_check(c, who, scope, budget)",
                 "gsr_debug_plane_times"):
        assert word in host, word
    ctx = open(os.path.join(CSRC, "gsr_api.cpp")).read()
    assert "c->pl.ev" in ctx                                           # the events go with the context


def test_the_chunk_constant_of_the_tests_is_the_source():
    import plane_reference as pr
    internal = open(os.path.join(CSRC, "gsr_internal.h")).read()
    assert int(re.search(r"constexpr uint32_t PLANE_CHUNK = (\d+);", internal).group(1)) == pr.CHUNK
    assert int(re.search(r"constexpr uint32_t PLANE_MAX_CHUNK_GROUPS = (\d+);", internal).group(1)) == pr.MAX_CHUNK_GROUPS
    assert int(re.search(r"constexpr uint32_t PLANE_MAX_HYPOTHESES = (\d+);", internal).group(1)) == pr.MAX_HYPOTHESES
    sizes = sorted({f[1].shape[0] for f in pr.families()})
    for m in (pr.CHUNK - 1, pr.CHUNK, pr.CHUNK + 1, 2 * pr.CHUNK + 1, 63, 64, 65, 255, 256, 257, 1, 2, 3):
        assert m in sizes, m
    assert sizes[-1] > pr.CHUNK * pr.MAX_CHUNK_GROUPS                  # one family makes a workgroup walk a second chunk
    assert {1, 63, 64, 65, 256, 257, 4096} <= {f[3] for f in pr.families()}
    assert max(f[1].shape[0] * f[3] for f in pr.families()) <= 8192 * 4096
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "PLANE_CHUNK = %d" % pr.CHUNK in design


def test_library_holds_the_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    assert len(set(re.findall(r"_ZN3gsr18k_plane_candidatesILb[01]EEEv\w*", out))) == 2    # the count and the scatter
    assert re.search(r"_ZN3gsr12k_plane_scanE\w+", out)
    assert re.search(r"_ZN3gsr18k_plane_hypothesesE\w+", out)
    assert len(set(re.findall(r"_ZN3gsr13k_plane_scoreILi(?:64|256)EEEv\w*", out))) == 2    # the narrow and the wide workgroup
    assert re.search(r"_ZN3gsr12k_plane_bestE\w+", out)
    assert re.search(r"_ZN3gsr14k_plane_selectE\w+", out)
    twin = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
    if os.path.exists(twin):
        t = subprocess.run(["strings", "-a", twin], capture_output=True, text=True).stdout
        assert "gsr_debug_bounds_plane" in t and "gsr_debug_bounds_plane" not in out


def test_host_file_compiles_clean_with_wall_wextra(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    obj = os.path.join(str(tmp_path), "gsr_plane.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-x", "hip", "-c",
                        os.path.join(CSRC, "gsr_plane.cpp"), "-o", obj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cpp_caller_lists_the_option():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "[--plane THRESHOLD[:HYPOTHESES]]" in r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    for word in ("gsr_fit_plane", "gsr_select_plane", "gsr_debug_plane_times", "candidates_ms", "score_ms", "\\\"tests\\\"", "tests_per_s", "inliers", "fit_equals_selection"):
        assert word in src, word


def test_documents_describe_the_calls():
    for name, words in (("README.md", ("gsr_fit_plane", "gsr_plane_inliers", "gsr_select_plane", "gsr_plane_alignment", "fitPlane", "selectPlane", "planeAlignment",
                                       "fit_plane", "select_plane", "plane_alignment", "--plane THRESHOLD[:HYPOTHESES]")),
                        ("DESIGN.md", ("\"Planes\"", "k_plane_candidates", "k_plane_hypotheses", "k_plane_score", "k_plane_best", "k_plane_select", "5.20", "8.o",
                                       "splitmix64", "GSR_NEIGHBOUR_DEFAULT_BUDGET", "gsr_plane_alignment"))):
        text = open(os.path.join(ROOT, name)).read()
        for w in words:
            assert w in text, (name, w)
