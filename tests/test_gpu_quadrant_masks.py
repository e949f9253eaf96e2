"""The compositor's staging masks on the device (k_blend: four separating axes; k_blend2: two), on frames of a few bins whose
splats sit where a mask that is too tight would lose a pixel: the coverage scenes of tests/test_gpu_blend.py, splats placed
THROUGH THE PROJECTION so that their outline passes a quadrant's corner pixel on a diagonal of their own axes, and two of the
saturation stacks (masks and the saturation skip drop quadrants of the same entries).  Every pixel against
tests/blend_reference.py's f64 value within its derived bound, coverage compared exactly: no mask, no tolerance beyond the
bound.  tests/test_quadrant_mask_reference.py holds the rule itself against brute force, without a GPU."""
import numpy as np
import pytest

import blend_reference as BR
import quadrant_mask_reference as QM
from depth_reference import coverage_q
from test_gpu_blend import Frame, _context, _ran_as, _render
from test_oracle_render import make_scene

pytestmark = pytest.mark.gpu

FRAMES = [(96, 96), (256, 96)]
FX, Z = 500.0, 5.0


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


def _scale_of(axis_px):
    """the scale of a splat whose projected semi-axis is axis_px long at depth Z: axis^2 = 2 ((2 s fx / z)^2 + 0.3)"""
    return float(np.sqrt(axis_px * axis_px / 2.0 - 0.3)) * Z / (2.0 * FX)


def corner_scene(oracle, W, H, seed, count=500):
    """(camera, splats, aimed pixels): splats whose outline passes the corner pixel of a quadrant at 45 degrees of their own
    axes, the quadrant lying beyond that pixel.  Placed in two passes: the first projection gives the axes the device will
    see (quaternion bytes and the 0.3 px^2 blur move them), the second puts the centre where THOSE axes ask for it."""
    rng = np.random.default_rng(seed)
    cam, to_world = BR.front_view(W, H, FX, Z)
    v, p, vp = cam.f32()
    shapes = []
    for k in range(count):
        a = float(np.exp(rng.uniform(np.log(1.2), np.log(20.0))))
        b = max(0.85, a * float(rng.uniform(0.05, 1.0)))
        shapes.append(dict(scale=(_scale_of(a), _scale_of(b), _scale_of(b)), rot=BR._rot_z(float(rng.uniform(0.0, np.pi))),
                           rgba=(255, 255, 255, int(rng.integers(40, 128))), dz=-1.5 + 3.0 * k / count,
                           qx=int(rng.integers(0, W // 8)), qy=int(rng.integers(0, H // 8)),
                           sw=float(rng.choice([-1.0, 1.0])), sn=float(rng.choice([-1.0, 1.0])),
                           t=float(rng.choice([0.0, 1e-5, 1e-4, 1e-3])) * float(rng.choice([-1.0, 1.0]))))
    centres = [(8 * s["qx"] + 4.0, 8 * s["qy"] + 4.0) for s in shapes]
    aimed = []
    for _ in range(2):
        splats = [dict(pos=to_world(cx, cy, s["dz"]), scale=s["scale"], rgba=s["rgba"], rot=s["rot"]) for s, (cx, cy) in zip(shapes, centres)]
        data, pos = make_scene(oracle, splats)
        rec = np.asarray(oracle.project(data, v, p, cam.fx, cam.fy, W, H)[0], np.float64).reshape(-1, 8)
        was, centres, aimed = centres, [], []
        for k, (s, rc) in enumerate(zip(shapes, rec)):
            M = np.array([[rc[2], rc[3]], [rc[4], rc[5]]])
            n = (M[0] + s["sw"] * M[1]) * s["sn"]                     # |vPosition . (1, sw)| grows along n: the quadrant lies there
            px, py = 8 * s["qx"] + (0 if n[0] > 0 else 7), 8 * s["qy"] + (0 if n[1] > 0 else 7)
            d = np.linalg.solve(M, np.sqrt(2.0) * s["sn"] * np.array([1.0, s["sw"]]))
            d *= 1.0 + s["t"] / np.hypot(*d)
            c = (px + 0.5 - d[0], py + 0.5 - d[1])
            if 1.0 <= c[0] <= W - 1.0 and 1.0 <= c[1] <= H - 1.0:     # (a centre off the frame is not projected: that splat stays put)
                centres.append(c)
                aimed.append((k, px, py))
            else:
                centres.append(was[k])
    return cam, splats, aimed


def _frame(oracle, cam, splats, W, H):
    data, pos = make_scene(oracle, splats)
    return Frame(oracle, data, pos, cam, W, H)


@pytest.fixture(scope="module")
def scenes_of(oracle):
    """name -> (Frame, aimed pixels or None), each built and referenced once"""
    cache = {}

    def get(name):
        if name not in cache:
            kind, W, H = name
            if kind == "coverage":
                cam, splats = BR.coverage_scene(W, H, [(0, 0, W, H)], seed=7 + W, per_region=500, giants=True)
                cache[name] = (_frame(oracle, cam, splats, W, H), None)
            elif kind == "corners":
                cam, splats, aimed = corner_scene(oracle, W, H, seed=3 + W)
                cache[name] = (_frame(oracle, cam, splats, W, H), aimed)
            else:
                cam, splats = BR.stack_scene(kind, {"grey": 768, "corner": 4100}[kind])
                cache[name] = (_frame(oracle, cam, splats, W, H), None)
        return cache[name]

    yield get
    cache.clear()


def _mask_counts(fr):
    """(covered, two-axis, four-axis) pairs over the frame's bins, and that neither rule loses a covered pair"""
    vis = fr.raw[:, 11] == 1
    rec = fr.rec[vis]
    cov = two = four = 0
    for bx, by in QM.bins_of(fr.W, fr.H):
        c, t, f = QM.covered(rec, bx, by), QM.two_axes(rec, bx, by), QM.four_axes(rec, bx, by)
        assert not (c & ~f).any() and not (f & ~t).any()
        cov += int(c.sum()); two += int(t.sum()); four += int(f.sum())
    return cov, two, four


def _images(gh, monkeypatch, fr, what, env=None, cover=True):
    """throughput (k_blend) with and without the saturation skip, and default (k_blend2 on these frames): each inside the bound"""
    imgs = {}
    for key, form, sat in (("throughput", "throughput", None), ("throughput-nosat", "throughput", "0"), ("default", "default", None)):
        e = dict(env or {}, **({"GSR_SATURATE": sat} if sat else {}))
        r, _ = _context(gh, monkeypatch, form, fr.W, fr.H, env=e)
        imgs[key] = _render(r, fr)
        wi = _ran_as(r, form, e)
        assert wi["waves_per_tile"] == (1 if form == "throughput" else 2), wi      # k_blend / k_blend2
        fr.check(imgs[key], (what, key), cover=cover)
        r.dispose()
    assert np.array_equal(imgs["throughput"], imgs["throughput-nosat"]), what
    return imgs


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_coverage_scenes_lie_inside_the_bound_under_both_masks(gh, monkeypatch, scenes_of, size):
    W, H = size
    fr, _ = scenes_of(("coverage", W, H))
    cov, two, four = _mask_counts(fr)
    assert cov > 2000 and four < two, (cov, two, four)
    assert BR.small_quadrant_pairs(fr.rec, fr.bbox, fr.order, W, H) >= 150
    _images(gh, monkeypatch, fr, "masks coverage %dx%d" % size)


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: "%dx%d" % s)
def test_outlines_through_quadrant_corners_on_a_diagonal(gh, monkeypatch, scenes_of, size):
    W, H = size
    fr, aimed = scenes_of(("corners", W, H))
    # the scene is what it claims: the aimed pixels lie at |vPosition| = 2 on either side, within a few 1e-3
    r = np.array([np.sqrt(float(coverage_q(fr.rec[k], np.array([px]), np.array([py]))[0, 0])) for k, px, py in aimed])
    close = np.abs(r - 2.0) <= 4e-3
    assert len(aimed) >= 250 and close.mean() >= 0.8 and (r[close] <= 2.0).mean() >= 0.2 and (r[close] > 2.0).mean() >= 0.2, (close.mean(), (r[close] <= 2.0).mean())
    cov, two, four = _mask_counts(fr)
    assert cov > 2000 and four < two - 100, (cov, two, four)       # the diagonal axes decide here
    _images(gh, monkeypatch, fr, "masks corners %dx%d" % size)


@pytest.mark.parametrize("kind", ["grey", "corner"])
def test_masks_and_saturation_drop_quadrants_of_the_same_entries(gh, monkeypatch, scenes_of, kind):
    W, H = BR.STACK_FRAME
    fr, _ = scenes_of((kind, W, H))
    ref = fr.refs[(0, 0, W, H)]
    if kind == "corner":      # the stack ends short of the central bin's corner pixels: their quadrants stay flagged and alive
        assert ref["kept"][32, 32] == 1 and ref["rgba"][32, 32, 0] > 0.5
    _images(gh, monkeypatch, fr, "masks stack %s" % kind, env={"GSR_LONG_ITEMS": "1"}, cover=False)
