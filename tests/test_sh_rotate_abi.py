"""Rotating SH coefficients, the part that needs no GPU: gsr_sh_rotation against the specification (tests/sh_rotate_reference.py),
the four entry points exported, prototyped and documented in include/gsplat_hip.h rule by rule, in the manner of tests/test_edit_abi.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import sh_rotate_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_sh_rotation", "gsr_scene_rotate_sh", "gsr_scene_rotate_selected_sh", "gsr_scene_bake_sh_frame")
TOL = 2.0 ** -40


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp = ctypes.c_void_p
    assert lib.gsr_sh_rotation.argtypes == [vp, vp]
    assert lib.gsr_scene_rotate_sh.argtypes == [vp, vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    assert lib.gsr_scene_rotate_selected_sh.argtypes == [vp, vp, vp]
    assert lib.gsr_scene_bake_sh_frame.argtypes == [vp, vp]
    assert (gh.GSR_SH_ALL, gh.GSR_SH_SELECTED) == (0, 1)
    # a NULL context is refused by the three context calls, a NULL pointer by the pure one
    q = (ctypes.c_double * 4)(0, 0, 0, 1)
    m = (ctypes.c_double * 83)()
    rows = ctypes.c_uint32(7)
    for call in (lambda: lib.gsr_scene_rotate_sh(None, ctypes.addressof(q), 0, ctypes.byref(rows)),
                 lambda: lib.gsr_scene_rotate_selected_sh(None, ctypes.addressof(q), None),
                 lambda: lib.gsr_scene_bake_sh_frame(None, ctypes.addressof(q)),
                 lambda: lib.gsr_sh_rotation(None, ctypes.addressof(m)), lambda: lib.gsr_sh_rotation(ctypes.addressof(q), None)):
        assert call() == -1
    assert rows.value == 7 and list(q) == [0, 0, 0, 1]


def test_the_matrices_are_the_specification():
    import gsplat_hip as gh
    rng = np.random.default_rng(41)
    qs = rng.standard_normal((200, 4))
    qs[100:] *= np.exp(rng.uniform(-6.0, 6.0, (100, 1)))          # non-unit ones: normalised in f64
    qs[np.arange(8), rng.integers(0, 4, 8)] = 0.0
    worst = 0.0
    for q in qs:
        for got, want in zip(gh.sh_rotation(q), ref.matrices(q)):
            assert got.shape == want.shape and got.dtype == np.float64
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.abs(got @ got.T - np.eye(got.shape[0])).max() <= TOL
    assert worst <= TOL, worst


def test_the_identity_is_exact_and_the_layout_is_row_major():
    import gsplat_hip as gh
    for q in ((0, 0, 0, 1), (0, 0, 0, -2.5)):
        for D in gh.sh_rotation(q):
            assert np.array_equal(D, np.eye(D.shape[0]))
    # a quarter turn about z takes x to y: B_3 = C1 x becomes B_1 = -C1 y, so c'_1 = -c_3; the transpose would give +c_3
    D1 = gh.sh_rotation((0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4)))[0]
    assert np.abs(D1 - np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])).max() <= TOL
    lib = gh.load_library()
    m = np.zeros(83)
    q = np.array([0.3, -0.2, 0.5, 0.7])
    assert lib.gsr_sh_rotation(q.ctypes.data, m.ctypes.data) == 0
    want = ref.matrices(q)
    assert np.abs(m - np.concatenate([w.reshape(-1) for w in want])).max() <= TOL


@pytest.mark.parametrize("q", [(0.0, 0.0, 0.0, 0.0), (float("nan"), 0.0, 0.0, 1.0), (0.0, float("inf"), 0.0, 1.0), (0.0, 0.0, -float("inf"), 0.0)])
def test_a_bad_quaternion_is_refused(q):
    import gsplat_hip as gh
    with pytest.raises(gh.GsplatError) as e:
        gh.sh_rotation(q)
    assert e.value.code == -1 and "gsr_sh_rotation" in str(e.value) and "finite and not zero" in str(e.value)
    lib = gh.load_library()
    m = np.full(83, 5.0)
    qa = np.array(q, dtype=np.float64)
    assert lib.gsr_sh_rotation(qa.ctypes.data, m.ctypes.data) == -1
    assert (m == 5.0).all()                                        # nothing written


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_SH_ALL 0u", "#define GSR_SH_SELECTED 1u",
                 "int gsr_sh_rotation(const double *q , double *m );",
                 "int gsr_scene_rotate_sh(gsr_ctx *ctx, const double *q , uint32_t scope , uint32_t *rows);",
                 "int gsr_scene_rotate_selected_sh(gsr_ctx *ctx, const double *q , const double *pivot );",
                 "int gsr_scene_bake_sh_frame(gsr_ctx *ctx, double *q_used );"):
        assert decl in flat, decl
    assert src.index("/* ---- editing the selection ----") < src.index("/* ---- rotating SH coefficients ----") < src.index("/* ---- growing the scene ----")
    m = re.search(r"/\* ---- rotating SH coefficients ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on rotating SH coefficients"
    doc = " ".join(m.group(0).replace(" * ", " ").split())
    for words in ("vertex.glsl.ts:72-98", "band 1 is -C1*y, -C1*z, +C1*x", "C2[0]*xy .. C2[4]*(xx-yy)", "C3[0]*y*(3xx-yy) .. C3[6]*x*(xx-3yy)",
                  "C0*c_0 + sum c_k B_k(d) + 0.5", "sum c'_k B_k(R d) = sum c_k B_k(d) for every unit d",
                  "the colour seen from d is the colour formerly seen from R^T d", "linv = R^T", "every D_l is orthogonal",
                  "pure host function that needs no GPU", "finite and non-zero", "|q| = sqrt(((xx+yy)+zz)+ww)", "row-major, one after the other",
                  "9 + 25 + 49 = 83", "x = y = z = 0 yields the exact identity", "24 Fibonacci-sphere directions", "phi = acos(1 - 2(i+0.5)/24)",
                  "theta = pi(1+sqrt 5)(i+0.5)", "hold to 2^-40",
                  "half 2j in the low 16 bits of word j", "M = (float)m, rounded once", "s = M[k][j0]*c[j0]; s = s + M[k][j]*c[j] with j ascending",
                  "rounded to nearest even", "subnormals kept", "overflow to infinity", "any NaN stored as 0x7e00", "Half 0 (DC) keeps its bits",
                  "All three bands are always rotated", "repeated truncation shrinks coefficients under repeated edits",
                  "selected splats without an SH row are not touched", "receives the number of rows rotated", "never reads or writes linv",
                  "GSR_OK, rows = 0, no kernel is launched", "An unknown scope or a bad q: GSR_ERR_ARG, nothing touched",
                  "ordered and marked exactly like gsr_scene_set_rgba_selected", "one call serves every member",
                  "the frame and the follow switch are untouched",
                  "gsr_scene_rotate_selected(q, pivot) followed by gsr_scene_rotate_sh(q, GSR_SH_SELECTED), as one edit",
                  "with q as given", "the coefficients use the normalised q", "provided the SH frame is the identity",
                  "a message naming gsr_scene_bake_sh_frame", "Without SH rows it is gsr_scene_rotate_selected", "keeps its refusal",
                  "s2 = (sum linv_ij^2) / 3", "max |(linv . linv^T)_ij / s2 - delta_ij| <= 2^-20", "det > 0", "a condition, not a measurement",
                  "a non-uniform scale has no rotation", "Q = linv / sqrt(s2)", "Shepperd's four branches",
                  "gsr_scene_rotate_sh(q_used, GSR_SH_ALL), and the frame becomes the identity", "q_used = (0, 0, 0, 1), nothing launched"):
        assert words in doc, words


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    assert list(inspect.signature(gh.sh_rotation).parameters) == ["q_xyzw"]
    sig = lambda name: inspect.signature(getattr(gh.HIPRenderer, name)).parameters
    assert list(sig("scene_rotate_sh")) == ["self", "q_xyzw", "selected"] and sig("scene_rotate_sh")["selected"].default is False
    assert list(sig("scene_rotate_selected_sh")) == ["self", "q_xyzw", "pivot"] and sig("scene_rotate_selected_sh")["pivot"].default is None
    assert list(sig("scene_bake_sh_frame")) == ["self"]


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    for f in ("gsr_sh_rotate.cpp", "k_sh_rotate.hip"):
        assert f in srcs and os.path.exists(os.path.join(CSRC, f)), f   # SRCS feeds the objects, the build id and the bounds build
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS := (.*)$", mk, flags=re.M).group(1)
    host = open(os.path.join(CSRC, "gsr_sh_rotate.cpp")).read()
    for word in ("edit_begin(c)", "edit_end(c)", "invalidate_members(c, true)", "launch_sh_rotate(", "launch_edit_rotate(", "quat_matrix(",
                 "sh_frame_is_identity()", "reset_sh_frame()", "gsr_rigid_decompose("):
        assert word in host, word
    kern = open(os.path.join(CSRC, "k_sh_rotate.hip")).read()
    for word in ("GSR_BOUNDS_DECL(sh_rotate)", "GSR_BOUND(sh_rotate, 0,", "GSR_BOUND(sh_rotate, 1,", "GSR_BOUND(sh_rotate, 2,", "k_sh_rotate",
                 "ShRotation M", "set_bit(words, nwords, i)", "(_Float16)s", "0x7e00u", '#include "k_splat_ops.h"'):
        assert word in kern, word
    assert "__shared__" not in kern
