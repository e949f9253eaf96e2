"""Shared scenes on the GPU (include/gsplat_hip.h, "shared scenes"): contexts that share a scene render bit for
bit what independent contexts render from copies of it, edits through any member land between the frames in flight, limitBox
through a member reaches all of them, leaving and destroying in any order, the refusals, and a context that never shares.

Every comparison is bit for bit against fresh, independent contexts that were given the same rows and the same edits through the
calls that existed before.  n = 5000 is a multiple of neither 256 nor 1024 (the projection's last workgroup and limitBox's last
block are partial); 200x120 and 96x64 leave the last bin column and row partial; in the SH variant splats 2500.. carry SH, a third
of them in each degree."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5000
BAND = np.array([2499, 3333, 4166], dtype=np.int32)
SIZE_A, SIZE_B = (200, 120), (96, 64)
KINDS = {"a": dict(size=SIZE_A), "b": dict(size=SIZE_B, throughput=True), "c": dict(size=SIZE_A, band=(32, 96))}
POSES = (5, 47, 83)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)
SCALE = (1.25, 0.75, 1.5)
HALF_BOX = (0.0, 100.0, -100.0, 100.0, -100.0, 100.0)
EMPTY_BOX = (50.0, 51.0, -100.0, 100.0, -100.0, 100.0)


@pytest.fixture(scope="module")
def gh():
    import gsplat_hip
    gsplat_hip.load_library()
    return gsplat_hip


@pytest.fixture(scope="module")
def material(gh):
    """(rows, rows of another scene, SH textures), built once and never changed"""
    rows = np.array(gh.synth.synth_rows(N, 41), dtype=np.uint8).reshape(-1)
    other = np.array(gh.synth.synth_rows(3001, 43), dtype=np.uint8).reshape(-1)
    rng = np.random.default_rng(47)
    tex = []
    for _ in range(3):
        c = rng.standard_normal(((N - 1 - int(BAND[0])) * 8, 2)) * 0.35
        tex.append(np.ascontiguousarray(gh.pack_half2x16(c[:, 0], c[:, 1]), dtype=np.uint32))
    for a in [rows, other] + tex:
        a.flags.writeable = False
    return rows, other, tex


def _make(gh, kind):
    k = KINDS[kind]
    return gh.HIPRenderer(k["size"][0], k["size"][1], band=k.get("band"), throughput=k.get("throughput", False))


def _owner(gh, material, kind, sh, rows=None, follow=False):
    """an independent context with a scene of its own"""
    r = _make(gh, kind)
    r.set_scene_rows(material[0] if rows is None else rows)
    if sh:
        r.set_sh(material[2], BAND)
    if follow:
        r.set_sh_follow(True)
    return r


def _members(gh, material, sh, follow=False):
    """A uploads; B (throughput, other size) and C (a band) share its scene"""
    a = _owner(gh, material, "a", sh, follow=follow)
    b, c = _make(gh, "b"), _make(gh, "c")
    b.share_scene(a)
    c.share_scene(a)
    return {"a": a, "b": b, "c": c}


def _camera(gh, r, pose):
    return gh.orbit_camera(pose, width=r.width, height=r.height)


def _enqueue(gh, r, pose):
    r.set_camera(_camera(gh, r, pose))
    r.render_async()


def _frame(gh, r, pose, sh=False):
    """what a frame leaves: pixels, depth order and (SH) the evaluated colours, as bits"""
    _enqueue(gh, r, pose)
    r.sync()
    out = [r.readPixelsFloat().view(np.uint32).copy()]
    if r.scene_count():   # (an empty scene has neither colours nor an order to read)
        if sh:
            out.append(r.read_sh_colors().view(np.uint32).copy())
        out.append(r.lastDepthIndex().copy())
    return out


def _same(x, y):
    return len(x) == len(y) and all(p.shape == q.shape and np.array_equal(p, q) for p, q in zip(x, y))


def _dispose(*rs):
    for r in rs:
        if isinstance(r, dict):
            _dispose(*r.values())
        else:
            r.dispose()


# ---- 1. a sharer renders what an owner renders ----
@pytest.mark.parametrize("sh", [False, True], ids=["rgba", "sh"])
def test_a_sharer_renders_what_an_owner_renders(gh, material, sh):
    m = _members(gh, material, sh)
    fresh = {k: _owner(gh, material, k, sh) for k in KINDS}
    try:
        sharing = [m[k].scene_sharing() for k in "abc"]
        assert sharing[0][0] == 3 and sharing[0] == sharing[1] == sharing[2]
        want = N * (28 + 32) + (3 * 32 * (N - 1 - int(BAND[0])) if sh else 0)
        assert sharing[0][1] == want
        assert fresh["a"].scene_sharing() == (1, want)
        for pose in POSES:
            for k in "abc":
                got, ref = _frame(gh, m[k], pose, sh), _frame(gh, fresh[k], pose, sh)
                assert got[0].any(), "an empty image compares nothing"
                assert _same(got, ref), (pose, k)
    finally:
        _dispose(m, fresh)


# ---- 2. edits land between frames, with frames in flight ----
def test_edits_land_between_the_frames_in_flight(gh, material):
    p1, p2, p3, p4 = 5, 47, 83, 110
    m = _members(gh, material, True, follow=True)
    a, b, c = m["a"], m["b"], m["c"]
    fresh = {k: _owner(gh, material, k, True, follow=True) for k in KINDS}
    try:
        a.open_delivery(3)
        # no sync() anywhere in this block
        _enqueue(gh, a, p1)
        s1 = a.deliver()
        _enqueue(gh, b, p2)
        c.scene_rotate(QUAT)
        _enqueue(gh, a, p3)
        s3 = a.deliver()
        b.scene_scale(SCALE)
        _enqueue(gh, c, p4)
        for r in (a, b, c):
            r.sync()
        got1 = a.acquire(s1)[1].copy()
        got3 = a.acquire(s3)[1].copy()
        a.release(s1)
        a.release(s3)
        got2 = b.readPixelsFloat().view(np.uint32).copy()
        got4 = c.readPixelsFloat().view(np.uint32).copy()
        col4 = c.read_sh_colors().view(np.uint32).copy()
        scenes = [r.read_scene() for r in (a, b, c)]

        # independent contexts, the same edits through the same calls, one frame each at the point it was enqueued
        fa, fb, fc = fresh["a"], fresh["b"], fresh["c"]
        _enqueue(gh, fa, p1); fa.sync()
        want1 = fa.readPixels().copy()
        _enqueue(gh, fb, p2); fb.sync()
        want2 = fb.readPixelsFloat().view(np.uint32).copy()
        fa.scene_rotate(QUAT)
        _enqueue(gh, fa, p3); fa.sync()
        want3 = fa.readPixels().copy()
        fc.scene_rotate(QUAT)
        fc.scene_scale(SCALE)
        _enqueue(gh, fc, p4); fc.sync()
        want4 = fc.readPixelsFloat().view(np.uint32).copy()
        wcol4 = fc.read_sh_colors().view(np.uint32).copy()
        assert want1.any() and want3.any() and not np.array_equal(want1, want3)
        assert np.array_equal(got1, want1), "A's first frame must see the scene as it was before the rotate"
        assert np.array_equal(got2, want2), "B's frame was enqueued before both edits"
        assert np.array_equal(got3, want3), "A's second frame sees the rotate and not the scale"
        assert np.array_equal(got4, want4) and np.array_equal(col4, wcol4), "C's frame sees both edits"
        ref = fc.read_scene()
        for s in scenes:
            for x, y in zip(s, ref):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.array_equal(a.sh_frame()[0], fc.sh_frame()[0]) and np.array_equal(b.sh_frame()[0], c.sh_frame()[0])
    finally:
        _dispose(m, fresh)


# ---- 3. limitBox through a member ----
def test_limit_box_through_a_member(gh, material):
    m = _members(gh, material, True, follow=True)
    a, b, c = m["a"], m["b"], m["c"]
    fresh = {k: _owner(gh, material, k, True, follow=True) for k in KINDS}
    try:
        for k in "abc":   # every member and every reference has a frame behind it when the edit arrives
            assert _same(_frame(gh, m[k], POSES[0], True), _frame(gh, fresh[k], POSES[0], True))
        a.depth_async()   # fine behind A's frame ...
        kept = b.scene_limit_box(HALF_BOX)
        assert N // 3 < kept < 2 * N // 3
        with pytest.raises(gh.GsplatError) as ei:   # ... and refused once the scene was edited behind it, through whichever member
            a.depth_async()
        assert ei.value.code == -1
        assert [r.scene_count() for r in (a, b, c)] == [kept] * 3
        for k in "abc":
            assert fresh[k].scene_limit_box(HALF_BOX) == kept
        tex, band = fresh["a"].read_scene_sh()
        assert tex[0].size and band[0] < kept - 1
        for r in (a, b, c):
            t, bd = r.read_scene_sh()
            assert np.array_equal(bd, band) and all(np.array_equal(x, y) for x, y in zip(t, tex))
        for pose in POSES[1:]:
            for k in "abc":
                got, ref = _frame(gh, m[k], pose, True), _frame(gh, fresh[k], pose, True)
                assert got[0].any() and _same(got, ref), (pose, k)
        # a second limitBox keeps nothing: every member renders the empty frame
        assert c.scene_limit_box(EMPTY_BOX) == 0
        for k in "abc":
            assert fresh[k].scene_limit_box(EMPTY_BOX) == 0 and m[k].scene_count() == 0
            got, ref = _frame(gh, m[k], POSES[0], True), _frame(gh, fresh[k], POSES[0], True)
            assert _same(got, ref) and not got[0].any(), k
            assert m[k].read_scene_sh()[0][0].size == 0
    finally:
        _dispose(m, fresh)


def test_new_sh_through_a_member_that_has_not_followed_a_limit_box_yet(gh, material):
    """limitBox through B, then new SH textures through A with no frame on A in between: A must still follow the limitBox (its
    sort's blocks, its binning plan) -- the generation the SH upload makes must not hide the one A has not adopted."""
    m = _members(gh, material, False)
    a, b, c = m["a"], m["b"], m["c"]
    fresh = {k: _owner(gh, material, k, False) for k in KINDS}
    try:
        for k in "abc":
            assert _same(_frame(gh, m[k], POSES[0]), _frame(gh, fresh[k], POSES[0]))
        kept = b.scene_limit_box(HALF_BOX)
        first = kept - 1500   # the last 1500 kept splats carry SH, 500 in each degree
        band = np.array([first - 1, first + 499, first + 999], dtype=np.int32)
        tex = [t[:1500 * 8] for t in material[2]]
        a.set_sh(tex, band)
        for k in "abc":
            assert fresh[k].scene_limit_box(HALF_BOX) == kept
            fresh[k].set_sh(tex, band)
        for pose in POSES[1:]:
            for k in "abc":
                got, ref = _frame(gh, m[k], pose, True), _frame(gh, fresh[k], pose, True)
                assert got[0].any() and _same(got, ref), (pose, k)
        assert a.stats()["n"] == kept
    finally:
        _dispose(m, fresh)


# ---- 4. leaving and lifetime ----
def test_leaving_and_lifetime(gh, material):
    rows, other, _ = material
    m = _members(gh, material, False)
    a, b, c = m["a"], m["b"], m["c"]
    fresh = {k: _owner(gh, material, k, False) for k in KINDS}
    fresh_other = _owner(gh, material, "b", False, rows=other)
    try:
        pose = POSES[1]
        want = {k: _frame(gh, fresh[k], pose) for k in KINDS}
        b.set_scene_rows(other)
        assert b.scene_sharing()[0] == 1 and a.scene_sharing()[0] == 2 and c.scene_sharing()[0] == 2
        assert b.scene_count() == other.size // 32 and a.scene_count() == N
        assert _same(_frame(gh, b, pose), _frame(gh, fresh_other, pose))
        assert _same(_frame(gh, a, pose), want["a"]) and _same(_frame(gh, c, pose), want["c"])
        # a refused upload (positions that differ from the data words) leaves the member where it was, still sharing
        data, pos, _, _ = c.read_scene()
        with pytest.raises(gh.GsplatError) as ei:
            c.set_raw_scene(data, pos + np.float32(1.0))
        assert ei.value.code == -4
        assert c.scene_sharing()[0] == 2 and a.scene_sharing()[0] == 2 and c.scene_count() == N
        assert _same(_frame(gh, c, pose), want["c"])
        # the context that uploaded goes first: the other member keeps rendering, and editing
        a.dispose()
        assert c.scene_sharing()[0] == 1
        assert _same(_frame(gh, c, pose), want["c"])
        c.scene_translate((0.25, -0.5, 1.0))
        fresh["c"].scene_translate((0.25, -0.5, 1.0))
        got, ref = _frame(gh, c, pose), _frame(gh, fresh["c"], pose)
        assert _same(got, ref) and not _same(got, want["c"])
    finally:
        _dispose(m, fresh, fresh_other)


# ---- 5. refusals ----
def test_refusals(gh, material):
    a, a2 = _owner(gh, material, "a", False), _owner(gh, material, "a", False)
    b, d = _make(gh, "b"), _make(gh, "b")
    try:
        with pytest.raises(gh.GsplatError) as ei:
            a.share_scene(a)
        assert ei.value.code == -1 and "itself" in str(ei.value)
        with pytest.raises(gh.GsplatError) as ei:
            b.share_scene(d)   # d was never given a scene
        assert ei.value.code == -1 and "never been given a scene" in str(ei.value)
        assert a.scene_sharing()[0] == 1 and b.scene_sharing()[0] == 1 and d.scene_sharing()[0] == 1
        b.share_scene(a)
        before = (a.scene_sharing(), b.scene_sharing())
        first = _frame(gh, b, POSES[0])
        b.share_scene(a)   # the scene it shares already: fine, and nothing changes (the frame behind it stays valid)
        assert (a.scene_sharing(), b.scene_sharing()) == before and before[0][0] == 2
        b.depth_async()
        assert _same(_frame(gh, b, POSES[0]), first)
        b.open_delivery(3)
        _enqueue(gh, b, POSES[1])
        s = b.deliver()
        b.acquire(s)
        b.share_scene(a)   # the scene it shares already is fine even with a frame held: nothing would change
        assert (a.scene_sharing(), b.scene_sharing()) == before
        with pytest.raises(gh.GsplatError) as ei:   # a held frame: as gsr_resize refuses
            b.share_scene(a2)
        assert ei.value.code == -1 and "held" in str(ei.value)
        assert b.scene_sharing()[0] == 2 and a2.scene_sharing()[0] == 1
        b.release(s)
        b.share_scene(a2)
        assert b.scene_sharing()[0] == 2 and a.scene_sharing()[0] == 1
        # a context that was given an empty scene HAS been given one
        d.set_raw_scene(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
        b.share_scene(d)
        assert b.scene_sharing()[0] == 2 and b.scene_count() == 0 and a2.scene_sharing()[0] == 1
        assert not _frame(gh, b, POSES[0])[0].any()
    finally:
        _dispose(a, a2, b, d)


# ---- 6. off means off ----
def test_a_context_that_never_shares_is_untouched(gh, material):
    """The projection stores a colour only for the splats it draws, so read_sh_colors() also holds what earlier poses left for the
    splats this pose does not draw: after one round over the poses that state repeats from round to round, and the rounds
    compared here all come behind such a round."""
    x = _owner(gh, material, "a", True)
    names = ("pixels", "sh colours", "depth index")
    try:
        assert x.scene_sharing()[0] == 1
        first = [_frame(gh, x, p, True) for p in POSES]
        before = [_frame(gh, x, p, True) for p in POSES]
        for p, q in zip(first, before):   # what a frame draws never depended on the frames before it
            assert np.array_equal(p[0], q[0]) and np.array_equal(p[2], q[2])
        m = _members(gh, material, True)
        try:
            for k in "abc":
                _frame(gh, m[k], POSES[0], True)
            m["b"].scene_rotate(QUAT)
            after = [_frame(gh, x, p, True) for p in POSES]
        finally:
            _dispose(m)
        assert x.scene_sharing()[0] == 1
        later = [_frame(gh, x, p, True) for p in POSES]
        for pose, b, a1, a2 in zip(POSES, before, after, later):
            for name, u, v, w in zip(names, b, a1, a2):
                print("pose %d %s: differing words while others share %d, after they are gone %d" % (pose, name, int((u != v).sum()), int((u != w).sum())))
                assert np.array_equal(u, v) and np.array_equal(u, w), (pose, name)
    finally:
        _dispose(x)
