"""Rotating SH coefficients through the Node host, on the GPU: renderer.rotateSH / rotateSelection(q, { sh: true }) / bakeSHFrame on a
real renderer (tests/js/sh_rotate_device_check.js, in a fresh child process) against the Python host given the same input and the
same walk: SHA-256 of the Scene's shs_rgb mirrors -- refreshed from the device on read -- and of the device copy's arrays after
every step, the rows rotated, the baked quaternion and the final frame."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sh_follow_reference as sf
import sh_rotate_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "js", "sh_rotate_device_check.js")
NODE = shutil.which("node")
N, W, H = 300, 64, 64
BAND = np.array([36, 123, 211], dtype=np.int32)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
QUAT2 = (-0.5, 0.5, 0.5, 0.5)
QUAT3 = (0.6, 0.0, -1.6, 0.4)
PIVOT = (0.25, -0.5, 0.125)
STEPS = ["start", "all", "selected", "selection_with_sh", "selection_with_sh_no_pivot", "selection_without_sh", "refused", "baked",
         "selection_with_sh_after_the_bake"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_node_host_equals_the_python_host(tmp_path):
    import gsplat_hip as gh
    addon = os.path.join(ROOT, "gsplat.js_amd", "js", "native", "gsplat_hip.node")
    assert NODE is not None and os.path.exists(addon), "node or the addon is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    rows = np.array(gh.synth.synth_rows(N, 23), dtype=np.uint8).reshape(-1)
    shs = (np.random.default_rng(31).standard_normal((N - 37, 48)) * 0.35).astype(np.float32)
    f, g = tmp_path / "s.splat", tmp_path / "s.shs"
    rows.tofile(f)
    shs.tofile(g)
    out = subprocess.run([NODE, DRIVER, str(f), str(g), str(W), str(H)] + [str(int(v)) for v in BAND], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    node = json.loads(out.stdout.strip().splitlines()[-1])
    assert [s["name"] for s in node["steps"]] == STEPS

    # the Python host, the same walk
    scene = gh.Scene()
    scene.bandsIndices = BAND.copy()
    scene.setData(rows, shs)
    mask = (7 * np.arange(N) + 3) % 10 < 3
    count = N - 37
    height = -(-(2 * count) // 2048)
    r = gh.HIPRenderer(W, H)
    want = []

    def keep(**extra):
        tex, band = r.read_scene_sh()
        assert list(band) == list(BAND)
        digests = []
        for t in tex:          # the Scene's layout: width * shHeight * 4 words, zeros behind the rows
            full = np.zeros(2048 * height * 4, dtype=np.uint32)
            full[:t.size] = t
            digests.append(_sha(full))
        want.append(dict(shs_rgb=digests, shHeight=height, geometry=[_sha(a) for a in r.read_scene()], **extra))
        return tex

    try:
        r.set_scene_rows(rows)
        r.set_sh(scene.shs_rgb, BAND)
        start = keep()
        all_rows = r.scene_rotate_sh(QUAT)
        turned = keep(rows=all_rows)
        assert all_rows == count
        assert all(np.array_equal(a, b) for a, b in zip(turned, ref.apply(start, BAND, None, ref.m32(gh.sh_rotation(QUAT)))))
        r.set_selection(mask)
        keep(rows=r.scene_rotate_sh(QUAT2, selected=True))
        assert want[-1]["rows"] == int(mask[37:].sum())
        r.scene_rotate_selected_sh(QUAT3, PIVOT)
        keep()
        r.scene_rotate_selected_sh(QUAT2)
        keep()
        r.scene_rotate_selected(QUAT, PIVOT)
        keep()
        assert want[-1]["shs_rgb"] == want[-2]["shs_rgb"] and want[-1]["geometry"] != want[-2]["geometry"]
        r.set_sh_follow(True)
        r.scene_rotate(QUAT)
        r.set_selection(mask)
        with pytest.raises(gh.GsplatError, match="gsr_scene_bake_sh_frame"):
            r.scene_rotate_selected_sh(QUAT2, PIVOT)
        frame = r.sh_frame()[0]
        keep(refused=True, shFrame=[float(v) for v in frame.reshape(-1)])
        q = r.scene_bake_sh_frame()
        assert np.array_equal(q, ref.bake(frame))
        keep(q=[float(v) for v in q], shFrame=[float(v) for v in sf.IDENTITY.reshape(-1)])
        assert np.array_equal(r.sh_frame()[0], sf.IDENTITY)
        r.scene_rotate_selected_sh(QUAT2, PIVOT)
        keep()
        cam = gh.Camera(position=(0.0, 0.0, -6.0), rotation=(0.0, 0.0, 0.0, 1.0), fx=40.0, fy=40.0)
        r.set_camera(cam)
        r.render_async()
        r.sync()
        pixels = _sha(r.readPixels())
        assert r.readPixels()[:, :, 3].any()
    finally:
        r.dispose()
    for got, exp, name in zip(node["steps"], want, STEPS):
        for key, value in exp.items():
            assert got[key] == value, (name, key)
    assert len({tuple(s["shs_rgb"]) for s in want}) == 7          # (every rotation really changed the mirrors: 9 steps, 2 of them leave them)
    assert node["drawn"] is True and node["pixels"] == pixels
