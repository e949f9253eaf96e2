"""Hidden splats in the hosts, without a GPU: the Python methods and their packing, Scene.setHidden against stub device scenes
(tests/js/hide_binding_check.js: once per distinct device copy, null = show all, no "change", its refusals), and the Node
renderer, typings, addon table and the C ABI benchmark carry the names."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "gsplat.js_amd", "js")
DRIVER = os.path.join(ROOT, "tests", "js", "hide_binding_check.js")
NODE = shutil.which("node")
NAMES_C = ("gsr_hide_selected", "gsr_hidden_set", "gsr_read_hidden", "gsr_select_hidden")

EXPECTED = [
    "no_device_throws", "set_once_per_distinct_copy", "both_copies_hold_the_mask", "returns_the_hidden_count", "arrays_unchanged_and_no_change_event",
    "null_shows_all", "short_mask_throws", "not_a_mask_throws", "device_without_hidden_set_throws", "diverged_copies_throw", "current_again_after_change",
]


class _Lib:
    """records the gsr_hidden_set / gsr_hide_selected / gsr_select_hidden calls the Python host makes"""

    def __init__(self):
        self.calls = []

    def gsr_hidden_set(self, ctx, words, nwords, op, count):
        got = None if words is None else np.ctypeslib.as_array((ctypes.c_uint32 * nwords).from_address(words)).copy()
        self.calls.append(("hidden_set", got, nwords, op))
        return 0

    def gsr_hide_selected(self, ctx, op, count):
        self.calls.append(("hide_selected", op))
        return 0

    def gsr_select_hidden(self, ctx, op, count):
        self.calls.append(("select_hidden", op))
        return 0



def _host(n):
    import gsplat_hip as gh
    r = object.__new__(gh.HIPRenderer)
    r._L, r._ctx, r._n = _Lib(), None, n
    r._count = lambda: n
    r._check = lambda rc: None
    return gh, r


def test_python_host_sends_the_specified_words_and_ops():
    import hide_reference as HR
    n = 1025
    gh, r = _host(n)
    Hs = np.random.default_rng(3).random(n) < 0.5
    r.set_hidden(Hs)
    r.set_hidden(HR.pack(Hs), op="add")                       # words as hidden_words() returns them
    r.set_hidden(words=HR.pack(Hs), op="intersect")
    r.set_hidden(None)                                        # show all
    r.hide_selected()
    r.hide_selected(op="subtract")
    r.select_hidden()
    r.select_hidden(op="add")
    c = r._L.calls
    for k, op in ((0, 0), (1, 1), (2, 3)):
        assert c[k][0] == "hidden_set" and np.array_equal(c[k][1], HR.pack(Hs)) and c[k][2] == -(-n // 32) and c[k][3] == op
    assert c[3] == ("hidden_set", None, 0, 0)
    assert c[4:] == [("hide_selected", 1), ("hide_selected", 2), ("select_hidden", 0), ("select_hidden", 1)]
    with pytest.raises(ValueError, match="one entry per splat"):
        r.set_hidden(np.zeros(n - 1, bool))
    with pytest.raises(ValueError, match="op must be one of"):
        r.hide_selected(op="toggle")


@pytest.fixture(scope="module")
def protocol():
    if NODE is None:
        pytest.skip("node is not installed")
    r = subprocess.run([NODE, DRIVER], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_driver_ran_every_check(protocol):
    assert protocol["checks"] == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_protocol(protocol, name):
    assert name in protocol["checks"] and name not in protocol["failed"]


def test_renderer_typings_addon_and_bench_carry_the_names():
    src = open(os.path.join(JS, "renderers", "HIPRenderer.js")).read()
    for word in ("this.hideSelection = (options)", "this.showAll = ()", "this.setHidden = (words, options)", "this.readHidden = ()", "this.selectHidden = (options)",
                 "setHidden: (words)", '"add", "op"'):
        assert word in src, word
    scene = open(os.path.join(JS, "core", "Scene.js")).read()
    assert "setHidden(mask)" in scene and "this._distinctDevices()) count = d.setHidden(mask)" in scene
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for word in ("hideSelection(options?: { op?: SelectOp }): number;", "showAll(): number;", "setHidden(words: Uint32Array | null, options?: { op?: SelectOp }): number;",
                 "readHidden(): Uint32Array;", "selectHidden(options?: { op?: SelectOp }): number;", "setHidden(mask: Uint32Array | null): number;",
                 "setHidden?(words: Uint32Array | null): number;"):
        assert word in dts, word
    addon = open(os.path.join(JS, "native", "addon.cc")).read()
    for name, fn in (("hideSelected", "HideSelected"), ("setHidden", "SetHidden"), ("readHidden", "ReadHidden"), ("selectHidden", "SelectHidden")):
        assert '{"%s", %s}' % (name, fn) in addon, name
    for fn in NAMES_C:
        assert fn + "(" in addon, fn
    bench = open(os.path.join(ROOT, "tools", "bench_cabi.cpp")).read()
    assert '"--hide"' in bench and "gsr_hidden_set(" in bench and '\\"hidden\\"' in bench

