"""HIPRenderer's cell methods without a GPU (tests/js/merge_binding_check.js): against a stub native layer the two methods reach the
addon with the header's flags and the documented defaults, bad arguments throw before the addon, the addon's refusals pass through;
renderer, typings and addon table carry the names, and the Python host has the same constants and signatures."""
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "merge_binding_check.js")
NODE = shutil.which("node")

EXPECTED = ["constants_follow_the_header", "cells_defaults_scopes_and_result", "merge_defaults_and_result", "bad_arguments_throw_before_the_addon",
            "addon_errors_pass_through"]


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
    for word in ("this.splatCells", "this.mergeCells", "vertexCount = r.count"):
        assert word in src, word
    dts = open(os.path.join(ROOT, "gsplat.js_amd", "js", "index.d.ts")).read()
    for word in ("splatCells(cell: number, options?: CellOptions & { cap?: number; leaders?: boolean }): SplatCells;",
                 "mergeCells(cell: number, options?: CellOptions): CellInfo & { count: number };",
                 "export interface CellOptions { scope?: NeighbourScope | NeighbourScope[]; budget?: number }",
                 "export interface SplatCells extends CellInfo { hist: Uint32Array; leader?: Uint32Array }"):
        assert word in dts, word
    addon = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    for name, fn in (("cells", "Cells"), ("mergeCells", "MergeCells")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for call in ("gsr_cells(c,", "gsr_scene_merge_cells(c,"):
        assert call in addon, call
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "renderer.mergeCells(0.05);" in readme and "r.scene_merge_cells(0.05)" in readme


def test_python_host_has_the_same_constants_and_signatures():
    import gsplat_hip as gh
    import merge_reference as mr
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert int(re.search(r"#define GSR_CELL_NONE\s+(0x[0-9a-f]+)u", header).group(1), 16) == gh.CELL_NONE == mr.NONE
    assert gh.NEIGHBOUR_MAX_CAP == mr.MAX_CAP and (gh.NEIGHBOUR_DEFAULT_BUDGET, gh.NEIGHBOUR_MAX_BUDGET) == (mr.DEFAULT_BUDGET, mr.MAX_BUDGET)
    sig = inspect.signature(gh.HIPRenderer.cells)
    assert list(sig.parameters)[1:] == ["cell", "cap", "scope", "leaders", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [64, (), False, None]
    sig = inspect.signature(gh.HIPRenderer.scene_merge_cells)
    assert list(sig.parameters)[1:] == ["cell", "scope", "budget"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [(), None]
    for bad in (0, 4096):
        with pytest.raises(ValueError):
            gh.HIPRenderer._cell_args(1.0, bad, None)
    with pytest.raises(ValueError):
        gh.HIPRenderer._cell_args(1.0, 8, -1)
    assert gh.HIPRenderer._cell_args(1, 4095, None) == (1.0, 4095, 0)
    assert [f[0] for f in gh.GsrCellInfo._fields_] == ["in_scope", "candidates", "cells", "merged_cells", "merged_members", "largest", "rows_after", "pad",
                                                       "pair_bound", "budget"]
    info = gh.GsrCellInfo(rows_after=7, pair_bound=1 << 40).as_dict()
    assert info["rows_after"] == 7 and info["pair_bound"] == 1 << 40 and "pad" not in info
