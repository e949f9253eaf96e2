"""HIPRenderer's plane methods without a GPU (tests/js/plane_binding_check.js): against a stub native layer the four methods reach
the addon with the header's flags and the documented defaults, bad arguments throw before the addon, the addon's refusals pass
through; renderer, typings and addon table carry the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "plane_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "fit_defaults_scopes_and_result", "nothing_found_is_a_null_plane", "inliers_flatten_the_planes",
    "select_defaults_are_everything_replace", "within_is_lo_minus_t_hi_t", "alignment_returns_a_quaternion_and_a_vector",
    "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
]


@pytest.fixture(scope="module")
def protocol():
    if NODE is None:
        pytest.skip("node is not installed")
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"], protocol["failed"]


def test_renderer_typings_and_addon_carry_the_names():
    src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "renderers", "HIPRenderer.js")).read()
    for word in ("this.fitPlane", "this.planeInliers", "this.selectPlane", "this.planeAlignment", "new Quaternion(r.q[0], r.q[1], r.q[2], r.q[3])"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("fitPlane(threshold: number, options?: PlaneFitOptions): PlaneFit;",
                 "planeInliers(planes: ArrayLike<Plane>, threshold: number, options?: { scope?: NeighbourScope | NeighbourScope[]; budget?: number }): Uint32Array;",
                 "selectPlane(plane: Plane, options?: { within?: number; lo?: number; hi?: number; op?: SelectOp }): number;",
                 "planeAlignment(plane: Plane, options?: { axis?: ArrayLike<number> | Vector3 }): { rotation: Quaternion; translation: Vector3 };",
                 "export interface PlaneFitOptions { hypotheses?: number; seed?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number; scores?: boolean }"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("fitPlane", "FitPlane"), ("planeInliers", "PlaneInliers"), ("selectPlane", "SelectPlane"), ("planeAlignment", "PlaneAlignment")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_fit_plane(c,", "gsr_plane_inliers(c,", "gsr_select_plane(c,", "gsr_plane_alignment(plane, axis,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "const { rotation, translation } = renderer.planeAlignment(fit.plane); scene.rotate(rotation); scene.translate(translation);" in readme
    assert "plane, info = r.fit_plane(0.01); q, t = r.plane_alignment(plane); r.scene_rotate(q); r.scene_translate(t)" in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import plane_reference as pr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_PLANE_MAX_HYPOTHESES (\d+)u", header).group(1)) == gh.PLANE_MAX_HYPOTHESES == pr.MAX_HYPOTHESES == 4096
    assert (pr.DEFAULT_BUDGET, pr.MAX_BUDGET) == (gh.NEIGHBOUR_DEFAULT_BUDGET, gh.NEIGHBOUR_MAX_BUDGET)
    sig = inspect.signature(gh.HIPRenderer.fit_plane)
    assert list(sig.parameters)[1:] == ["threshold", "hypotheses", "seed", "scope", "budget", "scores"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [512, 0, (), 0, False]
    sig = inspect.signature(gh.HIPRenderer.plane_inliers)
    assert list(sig.parameters)[1:5] == ["planes", "threshold", "scope", "budget"]
    assert [p.default for p in list(sig.parameters.values())[3:5]] == [(), 0]
    sig = inspect.signature(gh.HIPRenderer.select_plane)
    assert list(sig.parameters)[1:] == ["plane", "lo", "hi", "within", "op"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [-np.inf, np.inf, None, "replace"]
    sig = inspect.signature(gh.HIPRenderer.plane_alignment)
    assert list(sig.parameters) == ["plane", "axis"] and sig.parameters["axis"].default == (0, 1, 0)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            gh.HIPRenderer._plane_args(0.1, bad, 0, "hypotheses")
    with pytest.raises(ValueError):
        gh.HIPRenderer._plane_args(0.1, 8, -1, "hypotheses")
    assert gh.HIPRenderer._plane_args(1, 512, None, "hypotheses") == (1.0, 512, 0)
    d = gh.GsrPlaneInfo().as_dict()
    assert set(d) == {"in_scope", "nonfinite", "hypotheses", "degenerate", "found", "best", "triple", "inliers", "tests", "budget", "plane"}
    assert d["triple"] == (0, 0, 0) and d["plane"].dtype == np.float64 and d["plane"].shape == (4,)
    q, t = gh.HIPRenderer.plane_alignment((0, 0, 1, -0.5))             # a static method: no renderer, no device
    wq, wt = pr.alignment((0, 0, 1, -0.5))
    assert np.array_equal(q, wq) and np.array_equal(t, wt)
