"""SH colour that follows the scene through rotate / scale / limitBox, on the GPU ("SH frame"): the frame form
of the projection bit for bit against the specification (tests/sh_follow_reference.py), the SH compaction byte for byte, a
long-lived context against one created from the State alone, and the argument rules.

The scene is the smallest at which the compaction can still go wrong: 3 * 1024 + 17 splats are more than three 1024-lane
compaction workgroups, bandsIndices (1023, 1500, 2600) puts the first threshold on a workgroup's last lane and the others in
mid-block, x grows with the index (an x-interval keeps an index range) and y is scattered (a y-interval keeps a scattered subset)."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import history_trace as ht
import sh_follow_reference as ref

pytestmark = pytest.mark.gpu

TOL_EXACT = 2e-4
N, W, H = 3 * 1024 + 17, 256, 192
BAND = np.array([1023, 1500, 2600], dtype=np.int32)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
QUAT2 = (-0.5, 0.5, 0.5, 0.5)
SCALE = (1.25, 0.75, 1.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
NODE_DRIVER = os.path.join(ROOT, "tests", "js", "sh_follow_device_check.js")
NODE = shutil.which("node")
KINDS = {"default": {}, "band": {"band": (64, 192)}, "throughput": {"throughput": True}}
WIDE = 100.0


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def material(gh):
    """(rows, textures, camera) of the test scene, built once"""
    rows = np.array(gh.synth.synth_rows(N, 23), dtype=np.uint8).reshape(N, 32)
    p = rows[:, 0:12].copy().view(np.float32).reshape(N, 3)
    p[:, 0] = np.linspace(-2.0, 2.0, N).astype(np.float32)
    p[:, 2] *= np.float32(0.5)
    rows[:, 0:12] = p.view(np.uint8).reshape(N, 12)
    rng = np.random.default_rng(29)
    tex = []
    for _ in range(3):
        c = rng.standard_normal(((N - 1024) * 8, 2)) * 0.35
        tex.append(np.ascontiguousarray(gh.pack_half2x16(c[:, 0], c[:, 1]), dtype=np.uint32))
    cam = gh.orbit_camera(33, width=W, height=H)
    return rows.reshape(-1), tex, cam


def _context(gh, material, kind="default", follow=True, lib_path=None):
    rows, tex, _ = material
    r = gh.HIPRenderer(W, H, lib_path=lib_path, **KINDS[kind])
    r.set_scene_rows(rows)
    r.set_sh(tex, BAND)
    r.set_sh_follow(follow)
    return r


def _frame(r, cam):
    r.set_camera(cam)
    r.render_async()
    r.sync()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _columns(kind):
    x0, x1 = KINDS[kind].get("band", (0, W))
    return slice(x0, x1)


def _check_against_the_specification(oracle, r, cam, tex, band, frame, kind="default", least=300):
    """the context's next frame: colours of every drawn SH splat bit for bit, image within the project's tolerance of the oracle fed them"""
    _frame(r, cam)
    col, img = r.read_sh_colors(), r.readPixelsFloat()
    data, pos, _, _ = r.read_scene()
    n = pos.size // 3
    v, p, vp = cam.f32()
    orec, obbox, oraw = oracle.project(data, v, p, cam.fx, cam.fy, W, H, sh=tex, band=band)
    vis = (oraw[:, 11] == 1.0) & (np.arange(n) > band[0])
    assert vis.sum() >= least, vis.sum()
    want = ref.colours(oracle, tex, band, pos, v, frame, only=vis)
    assert np.array_equal(_bits(col[vis, :3]), _bits(want[vis]))
    oraw[vis, 7:10] = want[vis]
    oimg = oracle.render(oracle.sort(vp, pos)[0], oraw, orec, obbox, W, H, 1)
    cols = _columns(kind)
    assert np.abs(img[:, cols].astype(np.float64) - oimg[:, cols]).max() <= TOL_EXACT
    return want, vis


# ---- the frame form of the projection ----
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_frame_form_is_the_specification(gh, oracle, material, kind):
    _, tex, cam = material
    on, off = _context(gh, material, kind, True), _context(gh, material, kind, False)
    try:
        # an identity frame with follow on: the bits of a context that never opted in
        _frame(on, cam)
        _frame(off, cam)
        assert np.array_equal(_bits(on.read_sh_colors()), _bits(off.read_sh_colors()))
        assert np.array_equal(_bits(on.readPixelsFloat()), _bits(off.readPixelsFloat()))
        plain, vis = _check_against_the_specification(oracle, on, cam, tex, BAND, None, kind)
        # rotate, then scale on top of it
        on.scene_rotate(QUAT)
        frame = ref.frame_rotate(ref.IDENTITY, QUAT)
        assert np.array_equal(on.sh_frame()[0], frame) and on.sh_frame()[1] is True
        turned, vis2 = _check_against_the_specification(oracle, on, cam, tex, BAND, frame, kind)
        both = vis & vis2
        assert np.abs(turned[both] - plain[both]).max() > 0.05      # (the colours really moved with the scene)
        on.scene_scale(SCALE)
        frame = ref.frame_scale(frame, SCALE)
        assert np.array_equal(on.sh_frame()[0], frame)
        _check_against_the_specification(oracle, on, cam, tex, BAND, frame, kind)
        # follow off: the same edits leave the frame alone, and the colours are the stale ones of today
        off.scene_rotate(QUAT)
        assert np.array_equal(off.sh_frame()[0], ref.IDENTITY) and off.sh_frame()[1] is False
        _check_against_the_specification(oracle, off, cam, tex, BAND, None, kind)
    finally:
        on.dispose()
        off.dispose()


def test_frame_form_after_a_scale_alone(gh, oracle, material):
    _, tex, cam = material
    r = _context(gh, material)
    try:
        r.scene_scale(SCALE)
        _check_against_the_specification(oracle, r, cam, tex, BAND, ref.frame_scale(ref.IDENTITY, SCALE))
    finally:
        r.dispose()


# ---- compaction ----
def _x_of(material, i):
    return float(np.array(material[0]).reshape(N, 32)[i, 0:4].copy().view(np.float32)[0])


def _boxes(material):
    everything = (-WIDE, WIDE, -WIDE, WIDE, -WIDE, WIDE)
    scattered = (-WIDE, WIDE, -0.6, 0.9, -WIDE, WIDE)
    index_range = (_x_of(material, 700), _x_of(material, 2800), -WIDE, WIDE, -WIDE, WIDE)        # across all three thresholds
    prefix = (-WIDE, _x_of(material, 1023), -WIDE, WIDE, -WIDE, WIDE)                             # exactly the splats without SH
    nothing = (50.0, 60.0, -WIDE, WIDE, -WIDE, WIDE)
    return {"mixed": [everything, scattered, index_range, scattered], "prefix": [scattered, prefix], "nothing": [nothing]}


@pytest.mark.parametrize("sequence", ["mixed", "prefix", "nothing"])
def test_limit_box_compacts_the_sh_state(gh, oracle, material, sequence):
    _compaction(gh, oracle, material, sequence)


def test_bounds_twin_counts_nothing_over_the_compactions(gh, oracle, material):
    assert os.path.exists(BOUNDS_LIB), "the bounds-checked build is missing: run python -c 'import __graft_entry__ as g; g.build()'"
    L = gh.load_library(BOUNDS_LIB)
    for sequence in ("mixed", "prefix", "nothing"):
        _compaction(gh, oracle, material, sequence, lib_path=BOUNDS_LIB)
    for unit in (L.gsr_debug_bounds_scene_sh, L.gsr_debug_bounds_scene):
        buf = (ctypes.c_uint32 * 8)()
        assert unit(buf) == 0
        assert list(buf) == [0] * 8


def _compaction(gh, oracle, material, sequence, lib_path=None):
    _, tex, cam = material
    r = _context(gh, material, lib_path=lib_path)
    fresh = gh.HIPRenderer(W, H, lib_path=lib_path)
    try:
        r.scene_translate((0.0, 0.25, 0.0))     # (translate leaves the frame alone)
        r.scene_scale((1.0, 1.0, 1.25))         # x stays the index, the frame is not the identity
        frame = ref.frame_scale(ref.IDENTITY, (1.0, 1.0, 1.25))
        band = BAND
        for box in _boxes(material)[sequence]:
            pos = r.read_scene()[1]
            keep = ref.keep_mask(pos, box)
            tex, band, count = ref.compact_sh(tex, band, keep)
            assert r.scene_limit_box(box) == int(keep.sum())
            got_tex, got_band = r.read_scene_sh()
            assert list(got_band) == list(band)
            for a, b in zip(got_tex, tex):
                assert a.size == 8 * count and np.array_equal(a, b)
            if not keep.any():
                assert r.scene_count() == 0
                _frame(r, cam)
                assert not r.readPixelsFloat().any()
                continue
            # the next frame: a fresh context given the compacted scene, textures, thresholds and frame
            _frame(r, cam)
            fresh.set_scene_arrays(*r.read_scene())
            if count:
                assert np.array_equal(r.sh_frame()[0], frame)      # the frame survives the crop
                fresh.set_sh(tex, band)
                fresh.set_sh_frame(frame)
            _frame(fresh, cam)
            assert np.array_equal(_bits(r.readPixelsFloat()), _bits(fresh.readPixelsFloat()))
            if count:
                assert np.array_equal(_bits(r.read_sh_colors()), _bits(fresh.read_sh_colors()))
            else:
                with pytest.raises(gh.GsplatError):
                    r.read_sh_colors()
        if sequence == "mixed":
            assert 0 < count < N - 1024 and len(set(band)) == 3
            _check_against_the_specification(oracle, r, cam, tex, band, frame, least=100)
    finally:
        r.dispose()
        fresh.dispose()


def test_limit_box_without_follow_drops_the_sh_state(gh, material):
    r = _context(gh, material, follow=False)
    try:
        r.scene_limit_box(_boxes(material)["mixed"][1])
        tex, band = r.read_scene_sh()
        assert list(band) == [-1, -1, -1] and all(t.size == 0 for t in tex)
        with pytest.raises(gh.GsplatError):
            _frame(r, material[2])
            r.read_sh_colors()
    finally:
        r.dispose()


# ---- frame-to-frame state ----
def test_a_veteran_context_renders_as_one_made_from_the_state(gh, oracle):
    from test_gpu_history import observe, _same
    recipe = ("synth", N, 5, "rows")
    state = ht.State(W=W, H=H, scene=recipe, pose=7)
    rows = ht.scene_arrays(gh, recipe)[0]
    vet = ht.build(gh, state)

    def compare(state, tex, band, frame, follow, where):
        ht._frame(gh, vet, state, sync=True)
        a = observe(vet, state)
        a["SH colours"], a["SH frame"], a["SH state"] = vet.read_sh_colors(), vet.sh_frame(), vet.read_scene_sh()
        fresh = ht.build(gh, state)
        try:
            fresh.set_sh(tex, band)
            fresh.set_sh_follow(follow)
            fresh.set_sh_frame(frame)
            ht._frame(gh, fresh, state, sync=True)
            b = observe(fresh, state, a["pick points"])
            b["SH colours"], b["SH frame"], b["SH state"] = fresh.read_sh_colors(), fresh.sh_frame(), fresh.read_scene_sh()
        finally:
            fresh.dispose()
        for k in a:
            assert _same(a[k], b[k]) if k != "SH frame" else (np.array_equal(a[k][0], b[k][0]) and a[k][1] == b[k][1]), (where, k)

    try:
        tex, band = ht.sh_arrays(gh, (11, 0.33, 0.5, 0.8), N)
        vet.set_sh(tex, band)                                            # sh:on
        vet.set_sh_follow(True)                                          # follow:on
        vet.scene_rotate(QUAT)
        S = oracle.SceneState(rows)
        S.rotate(QUAT)
        tex, band, count = ref.compact_sh(tex, band, ref.keep_mask(S.positions, ht.BOX))
        assert 0 < count < N
        vet.scene_limit_box(ht.BOX)
        vet.scene_scale(SCALE)
        state = replace(state, transforms=(("rotate", QUAT), ("limit_box", ht.BOX), ("scale", SCALE)))
        frame = ref.frame_after(state.transforms)
        compare(state, tex, band, frame, True, "rotate, limit_box, scale with follow on")
        vet.set_sh_follow(False)                                         # follow:off: the frame stays where it is
        vet.scene_rotate(QUAT2)
        state = replace(state, transforms=state.transforms + (("rotate", QUAT2),), pose=8)
        compare(state, tex, band, frame, False, "rotate with follow off")
        tex, band = ht.sh_arrays(gh, (12, 0.25, 0.5, 0.75), vet.scene_count())
        vet.set_sh(tex, band)                                            # new coefficients: in the scene's frame as it stands
        assert np.array_equal(vet.sh_frame()[0], ref.IDENTITY)
        compare(replace(state, pose=9), tex, band, None, False, "gsr_set_scene_sh")
    finally:
        vet.dispose()


# ---- argument rules ----
def test_argument_rules(gh, material):
    _, tex, _ = material
    r = _context(gh, material)
    try:
        r.scene_rotate(QUAT)
        frame = r.sh_frame()[0]
        before = r.read_scene()
        for s in ((1.0, 0.0, 1.0), (float("nan"), 1.0, 1.0), (1.0, 1.0, float("inf"))):
            with pytest.raises(gh.GsplatError) as e:
                r.scene_scale(s)
            assert e.value.code == ht.GSR_ERR_ARG
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, r.read_scene()))
        bad = frame.copy()
        bad[1, 2] = float("inf")
        with pytest.raises(gh.GsplatError) as e:
            r.set_sh_frame(bad)
        assert e.value.code == ht.GSR_ERR_ARG
        assert np.array_equal(r.sh_frame()[0], frame) and not np.array_equal(frame, ref.IDENTITY)
        r.set_sh_frame(None)
        assert np.array_equal(r.sh_frame()[0], ref.IDENTITY)
        r.set_sh_frame(frame)
        r.set_sh(tex, BAND)                      # the frame is the identity after gsr_set_scene_sh
        assert np.array_equal(r.sh_frame()[0], ref.IDENTITY) and r.sh_frame()[1] is True
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        with pytest.raises(gh.GsplatError) as e:   # no SH state, no frame to set
            r.set_sh_frame(frame)
        assert e.value.code == ht.GSR_ERR_ARG
    finally:
        r.dispose()


# ---- the Node host ----
@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_node_host_equals_the_python_host(gh, material, tmp_path):
    """scene.shFollowsTransforms = true; rotate; limitBox; render on the Node host -- before the scene's first frame (JavaScript
    edits, then an upload with the frame) and attached (kernels, SH mirrors read back) -- against the Python host: SHA-256 of
    readPixels(), of the refreshed shs_rgb, and bandsIndices."""
    rows = material[0]
    shs = (np.random.default_rng(31).standard_normal((N - 1024, 48)) * 0.35).astype(np.float32)
    box = (-1.5, 1.25, -0.75, 1.5, -2.0, 2.0)
    fx = 150.0
    f, g = tmp_path / "s.splat", tmp_path / "s.shs"
    np.asarray(rows).tofile(f)
    shs.tofile(g)
    args = [str(v) for v in (f, g, W, H, repr(fx), *BAND)] + [repr(float(v)) for v in QUAT2 + box]
    out = subprocess.run([NODE, NODE_DRIVER] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    node = json.loads(out.stdout)
    # the Python host
    scene = gh.Scene()
    scene.bandsIndices = BAND.copy()
    scene.setData(rows, shs)
    r = gh.HIPRenderer(W, H)
    try:
        r.set_scene_rows(rows)
        r.set_sh(scene.shs_rgb, BAND)
        r.set_sh_follow(True)
        r.scene_rotate(QUAT2)
        kept = r.scene_limit_box(box)
        cam = gh.Camera(position=(0.0, 0.0, -6.0), rotation=(0.0, 0.0, 0.0, 1.0), fx=fx, fy=fx)
        r.set_camera(cam)
        r.render_async()
        r.sync()
        pixels = hashlib.sha256(r.readPixels().tobytes()).hexdigest()
        assert r.readPixels()[:, :, 3].any()
        tex, band = r.read_scene_sh()
        frame = r.sh_frame()[0]
    finally:
        r.dispose()
    count = tex[0].size // 8
    assert 0 < count < N - 1024 and 0 < kept < N
    height = -(-(2 * count) // 2048)
    digests = []
    for t in tex:          # the Scene's layout: width * shHeight * 4 words, zeros behind the rows
        full = np.zeros(2048 * height * 4, dtype=np.uint32)
        full[:t.size] = t
        digests.append(hashlib.sha256(full.tobytes()).hexdigest())
    for path in ("hostPath", "devicePath"):
        got = node[path]
        assert got["vertexCount"] == kept and got["shHeight"] == height and got["shDroppedOnDevice"] is False, path
        assert got["bandsIndices"] == [int(v) for v in band], path
        assert got["shs_rgb"] == digests, path
        assert np.array_equal(np.array(got["shFrame"], dtype=np.float64).reshape(3, 3), frame), path
        assert got["pixels"] == pixels, path
        assert got["pixelsAfterUpload"] == pixels, path
