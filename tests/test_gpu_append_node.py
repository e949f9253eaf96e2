"""Growing the scene through the Node host, on the GPU: a Scene bound to two real renderers that do not share a scene, grown through
Scene.duplicateSelection(mask) and Scene.append(other) -- both device copies follow and render what a fresh renderer renders -- its
arrays, read back from the device, against tests/append_reference.py bit for bit, and renderer.duplicateSelection() /
appendSelectionFrom() / reserveScene() / sceneCapacity() (tests/js/append_device_check.js, in a fresh child process)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import append_reference as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "append_device_check.js")
NODE = shutil.which("node")
N, M = 5000, 257
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)

EXPECTED = [
    "duplicate_reaches_both_device_copies", "vertex_count_follows_the_duplicate", "both_copies_render_the_grown_scene",
    "the_copies_are_the_selection_on_both_copies", "append_reaches_both_device_copies", "both_copies_render_the_appended_scene",
    "change_fired_as_a_device_edit_and_nothing_was_uploaded", "reserve_raises_the_capacity", "renderer_duplicate_returns_first_and_count",
    "a_renderer_duplicate_is_a_scene_edit", "append_selection_from_another_renderer", "both_copies_hold_the_same_scene_again",
    "nothing_selected_adds_nothing_and_keeps_the_frame",
]


def test_scene_bound_to_two_renderers_grows_on_both_device_copies(oracle, tmp_path):
    import gsplat_hip as gh
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    rows, other = gh.synth.synth_rows(N, 17), gh.synth.synth_rows(M, 5)
    rows_path, other_path, out_path = tmp_path / "rows.splat", tmp_path / "other.splat", tmp_path / "out.bin"
    rows_path.write_bytes(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    other_path.write_bytes(np.ascontiguousarray(other, dtype=np.uint8).tobytes())
    r = subprocess.run([NODE, DRIVER, str(rows_path), str(other_path), str(out_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["checks"] == EXPECTED
    assert out["failed"] == []
    # scene.data / positions / rotations / scales, read back from the device after either step, against the reference's bytes
    st, src = oracle.SceneState(rows), oracle.SceneState(other)
    for s in (st, src):
        s.rotate(Q0)
        s.scale(S0)
    sel = (7 * np.arange(N) + 3) % 5 < 2
    assert (out["n"], out["m"], out["k"]) == (N, M, int(sel.sum()))
    got = np.frombuffer(out_path.read_bytes(), dtype=np.uint32)
    at = 0
    for step, grow in (("duplicate", lambda: ar.duplicate(st, sel)), ("append", lambda: ar.append_selected(st, src, np.ones(M, dtype=bool)))):
        grow()
        for field, words in (("data", 8), ("positions", 3), ("rotations", 4), ("scales", 3)):
            ref = getattr(st, field).view(np.uint32)[:words * st.n]
            if field == "data":     # the device's export leaves word 3 of a row zero; the reference keeps what setData left there
                ref = ref.reshape(-1, 8).copy()
                assert not got[at:at + 8 * st.n].reshape(-1, 8)[:, 3].any()
                ref[:, 3] = 0
                ref = ref.reshape(-1)
            assert np.array_equal(got[at:at + words * st.n], ref), "%s: %s differs" % (step, field)
            at += words * st.n
    assert at == got.size
