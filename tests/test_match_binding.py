"""HIPRenderer's matching and registration methods without a GPU (tests/js/register_binding_check.js): against a stub native layer
the four methods reach the addon with the header's flags and the documented defaults, bad arguments throw before the addon, the
addon's refusals pass through; renderer, typings and addon table carry the names, and the Python host has the same constants and
signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "register_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "match_defaults_scopes_and_result", "select_defaults_are_everything_replace", "register_defaults_and_result",
    "status_names_follow_the_codes", "decompose_returns_a_quaternion_and_a_vector", "bad_arguments_throw_before_the_addon", "a_disposed_target_is_refused",
    "addon_errors_pass_through",
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
    for word in ("this.matchScene", "this.selectMatch", "this.registerTo", "this.rigidDecompose", "rotation: new Quaternion(r.q[0], r.q[1], r.q[2], r.q[3])",
                 "translation: new Vector3(r.t[0], r.t[1], r.t[2])", "const REGISTER_STATUS = [\"converged\", \"max_iterations\", \"too_few\"];"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("matchScene(target: HIPRenderer, radius: number, options?: MatchOptions & { sums?: boolean }): SceneMatch;",
                 "selectMatch(target: HIPRenderer, radius: number, options?: MatchOptions & { lo?: number; hi?: number; op?: SelectOp }): number;",
                 "registerTo(target: HIPRenderer, radius: number, options?: MatchOptions & { maxIterations?: number; tolerance?: number; history?: boolean }): Registration;",
                 "rigidDecompose(transform: RigidTransform): { rotation: Quaternion; translation: Vector3 };",
                 "export interface MatchOptions { transform?: RigidTransform | null; scope?: NeighbourScope | NeighbourScope[]; targetScope?: NeighbourScope | NeighbourScope[]; "
                 "budget?: number }",
                 "export type RegisterStatus = \"converged\" | \"max_iterations\" | \"too_few\";",
                 "export interface Registration { transform: Float64Array; rotation: Quaternion; translation: Vector3; status: RegisterStatus; iterations: number; pairs: number;"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("matchScene", "MatchScene"), ("selectMatch", "SelectMatch"), ("registerTo", "RegisterTo"), ("rigidDecompose", "RigidDecompose")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_match(c, a.target,", "gsr_select_match(c, a.target,", "gsr_register(c, a.target,", "gsr_rigid_decompose(M,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "const fit = renderer.registerTo(other, 0.25); scene.rotate(fit.rotation); scene.translate(fit.translation);" in readme
    assert "M, info = r.register(other, 0.25); q, t = gsplat_hip.rigid_decompose(M); r.scene_rotate(q); r.scene_translate(t)" in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import register_reference as rr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_MATCH_NONE (0x[0-9a-f]+)u", header).group(1), 16) == gh.MATCH_NONE == rr.NONE
    assert int(re.search(r"#define GSR_REGISTER_MAX_ITERATIONS_LIMIT (\d+)u", header).group(1)) == gh.REGISTER_MAX_ITERATIONS == rr.MAX_STEPS == 256
    assert gh.REGISTER_STATUS == {rr.CONVERGED: "converged", rr.MAX_ITERATIONS: "max_iterations", rr.TOO_FEW: "too_few"}
    assert (rr.DEFAULT_BUDGET, rr.MAX_BUDGET) == (gh.NEIGHBOUR_DEFAULT_BUDGET, gh.NEIGHBOUR_MAX_BUDGET)
    sig = inspect.signature(gh.HIPRenderer.match)
    assert list(sig.parameters)[1:9] == ["target", "radius", "transform", "scope", "target_scope", "idx", "d2", "sums"]
    assert [p.default for p in list(sig.parameters.values())[3:9]] == [None, (), (), True, True, False]
    sig = inspect.signature(gh.HIPRenderer.select_match)
    assert list(sig.parameters)[1:5] == ["target", "radius", "lo", "hi"] and {"transform", "scope", "target_scope", "op", "budget"} <= set(sig.parameters)
    assert (sig.parameters["lo"].default, sig.parameters["hi"].default, sig.parameters["op"].default) == (0.0, None, "replace")
    sig = inspect.signature(gh.HIPRenderer.register)
    assert list(sig.parameters)[1:7] == ["target", "radius", "transform", "max_iterations", "tolerance", "history"]
    assert [p.default for p in list(sig.parameters.values())[3:7]] == [None, 32, 2.0 ** -40, False]
    with pytest.raises(TypeError):
        gh.HIPRenderer._match_args(object(), 0.1, None)
    d = gh.GsrMatchInfo().as_dict()
    assert set(d) == {"in_scope", "nonfinite", "target_indexed", "matched", "pair_bound", "budget", "d2_min", "d2_max"} and isinstance(d["d2_min"], float)
    s = gh.GsrMatchSums().as_dict()
    assert s["pairs"] == 0 and s["sum"].dtype == np.float64 and s["sum"].shape == (16,)
    assert set(gh.GsrRegisterInfo().as_dict()) == {"status", "iterations", "pairs", "rms", "delta"}
    M = np.concatenate([rr.motion()[0], rr.motion()[1][:, None]], axis=1)
    q, t = gh.rigid_decompose(M)                                       # module level: no renderer, no device
    wq, wt = rr.rigid_decompose(M)
    assert np.array_equal(q, wq) and np.array_equal(t, wt)
    assert np.array_equal(gh.rigid_compose(rr.IDENTITY, M), M)
