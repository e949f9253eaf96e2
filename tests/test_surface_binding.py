"""HIPRenderer's point-to-plane methods without a GPU (tests/js/surface_binding_check.js): against a stub native layer registerTo
with residual "surface" and matchSurface reach the addon with the header's flags and the documented defaults, residual "point" is
the path of today, bad arguments throw before the addon, the addon's refusals pass through; renderer, typings and addon table carry
the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "surface_binding_check.js")
NODE = shutil.which("node")

EXPECTED = [
    "constants_follow_the_header", "residual_point_is_the_path_of_today", "residual_surface_defaults_and_result", "status_names_follow_the_codes",
    "match_surface_defaults_and_result", "surface_solve_is_a_module_function", "bad_arguments_throw_before_the_addon", "addon_errors_pass_through",
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
    for word in ("this.matchSurface", "this._n.registerSurface(this._h, ...args, ...surfaceNormals(o2), steps, tolerance, !!o2.history)",
                 "const SURFACE_STATUS = REGISTER_STATUS.concat([\"degenerate\"]);", "function surfaceSolve(sums)", "residual === \"surface\""):
        assert word in src, word
    index = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.js")).read()
    assert "surfaceSolve: surfaceSolve" in index
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("export interface SurfaceNormals { source?: \"own\" | \"knn\"; radius?: number; k?: number; budget?: number }",
                 "export type SurfaceRegisterStatus = RegisterStatus | \"degenerate\";", "export interface SurfaceRegistration {", "export interface SurfaceMatch {",
                 "residual: \"surface\"; normals?: SurfaceNormals;", "residual: \"point\";",
                 "matchSurface(target: HIPRenderer, radius: number, options?: MatchOptions & { normals?: SurfaceNormals }): SurfaceMatch;",
                 "export function surfaceSolve(sums: { surfacePairs: number; sums: ArrayLike<number> }): { transform: Float64Array; rms: number; degenerate: number };"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("matchSurface", "MatchSurface"), ("registerSurface", "RegisterSurface"), ("surfaceSolve", "SurfaceSolve")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_match_surface(c, a.target,", "gsr_register_surface(c, a.target,", "gsr_surface_solve(&ss,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "renderer.registerTo(other, 0.25, { residual: \"surface\" })" in readme
    assert "r.register_surface(other, 0.25, normals=dict(source=\"own\"))" in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import surface_reference as sr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_REGISTER_DEGENERATE (\d+)", header).group(1)) == sr.DEGENERATE == 3
    assert gh.REGISTER_SURFACE_STATUS == {sr.CONVERGED: "converged", sr.MAX_ITERATIONS: "max_iterations", sr.TOO_FEW: "too_few", sr.DEGENERATE: "degenerate"}
    sig = inspect.signature(gh.HIPRenderer.register_surface)
    assert list(sig.parameters)[1:8] == ["target", "radius", "normals", "transform", "max_iterations", "tolerance", "history"]
    assert [p.default for p in list(sig.parameters.values())[3:8]] == [None, None, 32, 2.0 ** -40, False]
    assert {"scope", "target_scope", "budget"} <= set(sig.parameters)
    sig = inspect.signature(gh.HIPRenderer.match_surface)
    assert list(sig.parameters)[1:5] == ["target", "radius", "normals", "transform"] and {"scope", "target_scope", "budget"} <= set(sig.parameters)
    with pytest.raises(TypeError):
        gh.HIPRenderer.match_surface(object.__new__(gh.HIPRenderer), object(), 0.1)
    s = gh.GsrSurfaceSums().as_dict()
    assert s["pairs"] == 0 and s["surface_pairs"] == 0 and s["sum"].dtype == np.float64 and s["sum"].shape == (29,)
    assert set(gh.GsrRegisterSurfaceInfo().as_dict()) == {"status", "iterations", "pairs", "surface_pairs", "rms", "surface_rms", "delta", "valid"}
    assert callable(gh.surface_solve)                                  # module level: no renderer, no device
