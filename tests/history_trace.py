"""What a frame may depend on (State), everything a host can do to a context between frames (operations), and sequences of
them (traces): the material of tests/test_gpu_history.py, which walks one long-lived context through a trace and compares every
frame, bit for bit, with the frame of a context created a moment ago from the State alone.

Pure Python and numpy: building and folding a trace needs no GPU (tests/test_history_trace.py); only `apply` and `build`
touch a renderer.  An operation is a tuple (kind, *arguments); a trace is a list of Step(op, check): after a checked step the
test renders the State's pose on both contexts and compares, an unchecked step is followed directly by the next operation."""
import os
import random
from collections import namedtuple
from dataclasses import dataclass, replace

import numpy as np

GSR_ERR_ARG, GSR_ERR_SCENE, GSR_ERR_OVERFLOW = -1, -4, -5   # include/gsplat_hip.h

Step = namedtuple("Step", "op check")


@dataclass(frozen=True)
class State:
    """Everything an observable of a frame may depend on -- and nothing else a context remembers."""
    kind: str = "default"            # "default" | "throughput": the two kinds of context bench.py and the hosts create
    timing: bool = False             # created with GSR_FLAG_TIMING
    knobs: tuple = ()                # ((environment name, value), ...): read once, when the context is created
    W: int = 640
    H: int = 480
    band: tuple = None               # (x0, x1) as the library keeps it (x1 clamped to W), None: the whole frame
    scene: tuple = ("synth", 2049, 5, "raw")   # recipe: ("synth", n, seed, form) | ("config", name, form); form "rows" | "raw"
    transforms: tuple = ()           # (("rotate" | "translate" | "scale" | "limit_box", values), ...) applied on the device, in order
    sh: tuple = None                 # (seed, f0, f1, f2): half textures from `seed`, band indices at those fractions of the count
    fade: tuple = (False, 0.0)       # (use, value) of gsr_set_depth_fade
    hit_alpha: float = 0.5
    ring: tuple = None               # (format, full_range, depth format | None, depth step): the open delivery ring
    pose: int = 0                    # camera k of the 120-frame orbit at this size


# Read-backs that must not disturb anything, and calls that are refused and must change nothing.
READBACKS = ("records", "keys", "bin_lists", "work_items", "depth_index", "read_depth", "pick", "stats")
REFUSALS = ("band_off_boundary", "size_zero", "positions_differ", "timing_interval_zero")
KINDS = ("camera", "same_pose", "burst", "sort_only", "readback", "scene", "resize", "band", "sh", "limit_box", "rotate",
         "translate", "scale", "fade", "hit_alpha", "depth_async", "timing_interval", "overflow_sync", "overflow_async",
         "ring_open", "ring_close", "deliver", "refused")
# operations after which the last frame's lists, records and planes are still the context's: only these may go unchecked
# (an unchecked step is followed directly by the next operation, which may be a read-back of that frame)
KEEPS_FRAME = ("camera", "same_pose", "burst", "sort_only", "readback", "fade", "hit_alpha", "timing_interval", "deliver", "depth_async")

# Ordered pairs of neighbours the tour must visit (tags as `tags` gives them), and why each is risky.
RISKY_PAIRS = (
    ("band:on", "band:off", "the full frame indexes rect[] / depth[] by splat where the band frame wrote survivors only"),
    ("band:off", "band:on", "the earlier band again: culled splats still hold the full frame's rectangles, packed slots its depths"),
    ("band:on", "band:move", "a splat culled now was a survivor a frame ago and keeps that rectangle"),
    ("band:on", "resize", "gsr_resize drops the band without a gsr_set_band: the planes' fill key and the survivor buffers stay"),
    ("sort_only", "resize", "the sort-only frames' slot sets and parity meet a new bin grid"),
    ("sort_only", "readback", "a read-back directly behind a sort-only frame reads the render frame's buffers, not the sort's"),
    ("sort_only", "scene", "the slot set the last k_depth_key reset belongs to a scene that is gone"),
    ("scene:empty", "sort_only", "the parity does not move on an empty scene: the same slot set twice"),
    ("overflow_sync", "scene", "a regrown list, then gsr_set_scene sets the capacity back to 'by the scene'"),
    ("overflow_async", "scene", "dropped frames and a sticky device counter, then every per-splat buffer is new"),
    ("overflow_async", "band:on", "max_items was reset by the regrowth; the band's grid sizes the items anew"),
    ("readback:records", "camera", "k_project_key ran a second time over the render frames' slot set and the live rec / rect buffers"),
    ("readback:records", "same_pose", "... and the next frame is a graph replay with nothing rewritten but the camera"),
    ("burst", "readback:keys", "three frames in flight, then the keys of the last one"),
    ("sh:on", "limit_box", "the compaction renumbers the splats: SH rows and shcol[] of the old numbering must go"),
    ("limit_box", "sh:on", "SH for a scene whose count shrank while every per-splat buffer kept its size"),
    ("sh:on", "sh:off", "rgb8 records again after RGB8_IN_SHCOL ones"),
    ("scene:shrink", "camera", "buffers sized for the larger scene: the tail of depth[] / keys / rect[] is the old scene's"),
    ("scene:grow", "camera", "every per-splat buffer is new, the bin table may not be"),
    ("scene:rows", "scene:raw", "rotations / scales are dropped; transforms are refused from here on"),
    ("scene:raw", "scene:rows", "and allocated again"),
    ("resize:shrink", "resize:grow", "the original size again: framebuffer, planes and per-bin arrays were never shrunk"),
    ("ring_open", "resize", "the ring is reallocated at the new size and keeps its format"),
    ("resize", "deliver", "the first delivery into the new blocks"),
    ("ring_close", "ring_open", "another format in the slots' place"),
    ("hit_alpha", "depth_async", "planes cached for a frame_serial were cut at the old threshold"),
    ("depth_async", "camera", "the planes on the device belong to the frame before"),
    ("timing_interval", "camera", "individual launches with events, then graph replays, alternating"),
    ("fade:on", "fade:off", "the fade is part of the camera argument of the one node a replay rewrites"),
    ("refused", "camera", "a call that failed must have changed nothing the next frame reads"),
)


# ---------------------------------------------------------------------------------------------------------------------------
# State arithmetic (pure)
# ---------------------------------------------------------------------------------------------------------------------------
def scene_n(recipe):
    if recipe[0] == "config":
        from gsplat_hip import synth
        return synth.CONFIGS[recipe[1]]["n"]
    return recipe[1]


def scene_form(recipe):
    return recipe[-1]


def fold(state, op):
    """The State after `op` (what the library documents; the GPU tests check that the contexts agree)."""
    kind, a = op[0], op[1:]
    if kind in ("camera",):
        return replace(state, pose=a[0])
    if kind == "burst":
        return replace(state, pose=a[-1])
    if kind == "overflow_async":
        return replace(state, pose=a[-1])
    if kind == "scene":
        return replace(state, scene=a[0], transforms=(), sh=None)
    if kind == "resize":
        return replace(state, W=a[0], H=a[1], band=None)          # (gsr_resize drops the band)
    if kind == "band":
        return replace(state, band=None if a == (0, 0) else (a[0], min(a[1], state.W)))
    if kind == "sh":
        return replace(state, sh=a[0])
    if kind == "limit_box":
        return replace(state, transforms=state.transforms + (("limit_box", a[0]),), sh=None)   # (the compaction drops the SH state)
    if kind in ("rotate", "translate", "scale"):
        return replace(state, transforms=state.transforms + ((kind, a[0]),))
    if kind == "fade":
        return replace(state, fade=(bool(a[0]), float(a[1])))
    if kind == "hit_alpha":
        return replace(state, hit_alpha=float(a[0]))
    if kind == "ring_open":
        return replace(state, ring=tuple(a))
    if kind == "ring_close":
        return replace(state, ring=None)
    assert kind in KINDS, op
    return state      # same_pose, sort_only, readback, depth_async, timing_interval, overflow_sync, deliver, refused


def fold_all(state, trace):
    for st in trace:
        state = fold(state, st.op)
    return state


def tags(op, before):
    """The names an operation goes by in RISKY_PAIRS: its kind, and kind:variant where the variant matters."""
    kind, a = op[0], op[1:]
    out = {kind}
    if kind == "band":
        out.add("band:off" if a == (0, 0) else "band:move" if before.band is not None else "band:on")
        if a != (0, 0):
            out.add("band:on")
    elif kind == "scene":
        n0, n1 = scene_n(before.scene), scene_n(a[0])
        out.add("scene:" + scene_form(a[0]))
        if n1 == 0:
            out.add("scene:empty")
        if n1 > n0:
            out.add("scene:grow")
        if n1 < n0:
            out.add("scene:shrink")
    elif kind == "resize":
        p0, p1 = before.W * before.H, a[0] * a[1]
        out.add("resize:grow" if p1 > p0 else "resize:shrink")
    elif kind == "sh":
        out.add("sh:on" if a[0] else "sh:off")
    elif kind == "fade":
        out.add("fade:on" if a[0] else "fade:off")
    elif kind in ("readback", "refused"):
        out.add(kind + ":" + a[0])
    return out


def pairs_in(state, trace):
    """every (tag, tag) of two neighbouring operations of the trace"""
    seen, prev = set(), None
    for st in trace:
        t = tags(st.op, state)
        if prev is not None:
            seen.update((x, y) for x in prev for y in t)
        prev, state = t, fold(state, st.op)
    return seen


def into_band(state, x, y):
    """a pixel of the frame moved into the State's band (gsr_pick refuses pixels outside it)"""
    if state.band is None:
        return (x, y)
    return (state.band[0] + x % (state.band[1] - state.band[0]), y)


def bins_of(W, H, band=None):
    nbx, nby = -(-W // 32), -(-H // 32)
    if band:
        return (min(-(-band[1] // 32), nbx) - band[0] // 32) * nby
    return nbx * nby


# ---------------------------------------------------------------------------------------------------------------------------
# Traces
# ---------------------------------------------------------------------------------------------------------------------------
def _band_for(W):
    x0 = (W // 3) // 32 * 32
    return (x0, min(W, x0 + max(32, (W // 4) // 32 * 32 + 17)))     # (x1 off a bin boundary: the last bin column is partial)


BOX = (-1.25, 1.5, -2.0, 1.0, -1.5, 1.25)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)


def tour(band_context=False):
    """The fixed trace: every operation, every read-back and refusal, every pair of RISKY_PAIRS, sizes on both sides of the 4096-bin
    boundary (two-level binning above it, two compositor waves per tile up to it) and scene sizes 0 .. 3.2 M (both keys-per-block
    steps and the bucket order's limit).  band_context: the trace of a context created with a band -- gsr_resize drops the band,
    so every resize is followed by a gsr_set_band for the new width."""
    C, N = True, False
    t = []

    def add(*op, check=C):
        t.append(Step(tuple(op), check))

    def size(W, H):
        add("resize", W, H)
        if band_context:
            add("band", *_band_for(W))

    # cameras, read-backs, sort-only frames on the first scene (contexts with stage events: every other frame carries them, the
    # others are graph replays)
    add("timing_interval", 2)
    add("camera", 7)
    add("same_pose")
    add("burst", 8, 9, 10, check=N)
    add("readback", "keys")
    add("readback", "records", check=N)
    add("camera", 11)                                   # records -> the next frame (individual launches or a first capture)
    add("readback", "records", check=N)
    add("same_pose")                                    # records -> graph replay
    for which in ("bin_lists", "work_items", "depth_index", "read_depth", "pick", "stats"):
        add("readback", which, check=N)
    add("sort_only", 1, 30, check=N)
    add("readback", "records")
    add("sort_only", 2, 31, check=N)
    add("readback", "depth_index")
    # band on, moved, off, on again with the earlier band
    add("band", 192, 448)
    add("readback", "records", check=N)
    add("camera", 12)
    add("band", 320, 600)
    add("band", 96, 300)
    add("band", 0, 0)
    add("band", 192, 448)
    add("sort_only", 1, 33)
    add("band", 0, 0)
    if band_context:
        add("band", 192, 448)
    # scenes of other sizes, growing and shrinking, rows and raw
    add("scene", ("synth", 0, 1, "raw"))
    add("sort_only", 2, 34, check=N)
    add("scene", ("synth", 1, 2, "rows"))
    add("scene", ("synth", 63, 3, "raw"))
    add("scene", ("synth", 70000, 4, "rows"))
    add("camera", 13)
    add("scene", ("synth", 2049, 5, "raw"))
    add("camera", 14)
    add("scene", ("synth", 300000, 6, "raw"))
    add("camera", 15)
    add("scene", ("synth", 3200000, 8, "rows"))          # above 3 << 20: 4096 keys per block, the LSD order only
    add("camera", 16)
    add("scene", ("config", "C1", "rows"))
    add("camera", 17)
    # transforms, SH, limit box
    add("rotate", QUAT)
    add("translate", (0.25, -0.125, 0.5))
    add("scale", (1.25, 0.75, 1.0))
    add("sh", (11, 0.0, 0.25, 0.5))
    add("camera", 18)
    add("sh", (12, 0.5, 0.5, 0.75))
    add("sh", None)
    add("sh", (11, 0.0, 0.25, 0.5))
    add("limit_box", BOX)
    add("sh", (13, 0.0, 0.5, 0.5))
    add("camera", 19)
    # depth fade, hit alpha, depth planes
    add("fade", True, 0.3)
    add("fade", False, 0.0)
    add("fade", True, 0.8)
    add("hit_alpha", 0.9)
    add("depth_async", False)
    add("camera", 20)
    add("depth_async", True)
    add("hit_alpha", 0.25)
    add("fade", False, 0.0)
    # stage events and graph replays, alternating
    add("timing_interval", 2)
    add("camera", 21)
    add("same_pose")
    add("timing_interval", 0xffffffff)
    add("camera", 22)
    add("timing_interval", 1)
    add("camera", 23)
    # sizes: odd, across the 4096-bin boundary in both directions, a shrink followed by the original size
    add("sort_only", 1, 35, check=N)
    size(333, 219)
    add("band", 64, 200)
    size(640, 480)
    size(2048, 2048)                                     # 4096 bins: one-level binning, two waves per tile (default contexts)
    size(2080, 2048)                                     # 4160 bins: two-level, one wave per tile
    add("camera", 24)
    size(2048, 2048)
    size(3840, 2160)
    add("band", 1728, 2208)                              # a band on a 4K frame: survivor sort and gather
    add("camera", 25)
    add("band", 0, 0)
    if band_context:
        add("band", 1728, 2208)
    size(1279, 717)
    size(640, 480)
    # list overflow: repaired by sync; three frames queued behind it
    add("scene", ("synth", 70000, 4, "raw"))
    add("overflow_sync", 2048)
    add("scene", ("synth", 20000, 9, "rows"))
    add("overflow_async", 2048, 40, 41, 42)
    add("band", 192, 448)
    add("overflow_async", 1024, 43, 44, 45)
    add("scene", ("synth", 70000, 4, "rows"))
    add("band", 0, 0)
    if band_context:
        add("band", 192, 448)
    # delivery rings
    add("ring_open", "rgba8", False, None, 1)
    add("deliver")
    add("resize", 801, 601)
    add("deliver")
    if band_context:
        add("band", *_band_for(801))
    add("ring_close")
    add("ring_open", "nv12", False, None, 1)
    add("deliver", check=N)
    add("camera", 26)
    add("ring_close")
    add("ring_open", "i420", True, "u16", 2)
    size(640, 480)
    add("deliver")
    add("ring_close")
    add("ring_open", "rgba8", False, "f32", 1)
    add("camera", 27)
    add("ring_close")
    add("ring_open", "nv12", True, "u16", 1)
    add("camera", 28)
    add("ring_close")
    add("ring_open", "rgba8", False, "f32", 2)
    add("camera", 29)
    add("ring_close")
    # refused calls
    add("sh", (14, 0.0, 0.25, 0.5))
    for which in REFUSALS:
        add("refused", which)
        add("camera", 50 + REFUSALS.index(which))
    return t


WALK_SIZES = ((640, 480), (333, 219), (900, 700), (64, 64), (801, 601), (512, 384), (160, 96))
WALK_SCENES = (0, 1, 63, 2049, 20000, 7000, 300, 12000)
WALK_RINGS = (("rgba8", False, None, 1), ("nv12", False, None, 1), ("i420", True, None, 1), ("rgba8", False, "u16", 1),
              ("nv12", True, "f32", 2), ("i420", False, "u16", 2), ("rgba8", False, "f32", 1))


def _gen(kind, s, rng):
    """operations that perform one `kind` from State `s` (a prelude where the kind needs one: rows for a transform, a ring for a delivery)"""
    pose = rng.randrange(120)
    rows_scene = ("scene", ("synth", rng.choice((2049, 7000, 20000)), rng.randrange(1, 50), "rows"))
    need_rows = [] if scene_form(s.scene) == "rows" else [rows_scene]
    if kind == "camera":
        return [("camera", pose)]
    if kind == "same_pose":
        return [("same_pose",)]
    if kind == "burst":
        return [("burst", pose, (pose + 1) % 120, (pose + 2) % 120)]
    if kind == "sort_only":
        return [("sort_only", rng.choice((1, 2)), pose)]
    if kind == "readback":
        return [("readback", rng.choice(READBACKS))]
    if kind == "scene":
        return [("scene", ("synth", rng.choice(WALK_SCENES), rng.randrange(1, 50), rng.choice(("rows", "raw"))))]
    if kind == "resize":
        return [("resize",) + rng.choice([z for z in WALK_SIZES if z != (s.W, s.H)])]
    if kind == "band":
        if s.band is not None and rng.random() < 0.4:
            return [("band", 0, 0)]
        x0 = rng.randrange(0, max(1, (s.W - 1) // 32 + 1)) * 32
        return [("band", x0, x0 + rng.choice((32, 64, 100, 257, 10000)))]
    if kind == "sh":
        if s.sh is not None and rng.random() < 0.4:
            return [("sh", None)]
        f = sorted(rng.choice((0.0, 0.25, 0.5, 0.75)) for _ in range(3))
        return [("sh", (rng.randrange(1, 99), f[0], f[1], f[2]))]
    if kind == "limit_box":
        return need_rows + [("limit_box", tuple(v * rng.choice((0.75, 1.0, 1.5)) for v in BOX))]
    if kind == "rotate":
        q = [rng.uniform(-1, 1) for _ in range(4)]
        ln = sum(v * v for v in q) ** 0.5 or 1.0
        return need_rows + [("rotate", tuple(v / ln for v in q))]
    if kind == "translate":
        return need_rows + [("translate", tuple(rng.choice((-0.5, -0.125, 0.0, 0.25, 0.5)) for _ in range(3)))]
    if kind == "scale":
        return need_rows + [("scale", tuple(rng.choice((0.75, 1.0, 1.25)) for _ in range(3)))]
    if kind == "fade":
        return [("fade", False, 0.0)] if s.fade[0] and rng.random() < 0.5 else [("fade", True, rng.choice((0.2, 0.5, 0.8)))]
    if kind == "hit_alpha":
        return [("hit_alpha", rng.choice([a for a in (0.1, 0.25, 0.5, 0.9, 1.0) if a != s.hit_alpha]))]
    if kind == "depth_async":
        return [("depth_async", rng.random() < 0.5)]
    if kind == "timing_interval":
        return [("timing_interval", rng.choice((1, 2, 3, 0xffffffff)))]
    if kind == "overflow_sync":
        return [("overflow_sync", rng.choice((1024, 2048)))]
    if kind == "overflow_async":
        return [("overflow_async", rng.choice((1024, 2048)), pose, (pose + 5) % 120, (pose + 10) % 120)]
    if kind == "ring_open":
        return ([("ring_close",)] if s.ring else []) + [("ring_open",) + rng.choice([g for g in WALK_RINGS if g != s.ring])]
    if kind == "ring_close":
        return ([] if s.ring else [("ring_open",) + rng.choice(WALK_RINGS)]) + [("ring_close",)]
    if kind == "deliver":
        return ([] if s.ring else [("ring_open",) + rng.choice(WALK_RINGS)]) + [("deliver",)]
    if kind == "refused":
        return [("refused", rng.choice(REFUSALS))]
    raise AssertionError(kind)


def walk(seed, steps, start=State()):
    """A seeded random walk over the same operations with cheap States (<= 20 000 splats, <= 900 x 700).  The kinds are dealt like
    cards -- one shuffled deck after another -- so that a walk of twice as many steps as there are kinds and preludes holds every
    kind; walk(seed, k) is the first k steps of walk(seed, k + 1), so a failure at step k replays as walk(seed, k + 1)."""
    rng = random.Random(seed)
    t, s = [], start
    while len(t) < steps:
        deck = list(KINDS)
        rng.shuffle(deck)
        for kind in deck:
            for op in _gen(kind, s, rng):
                check = not (op[0] in KEEPS_FRAME and rng.random() < 0.3)
                t.append(Step(op, check))
                s = fold(s, op)
    return t[:steps]


def describe(trace, upto=None):
    return "; ".join("%d:%s%s" % (i, " ".join(str(v) for v in st.op), "" if st.check else " (unchecked)")
                     for i, st in enumerate(trace[:upto]))


# ---------------------------------------------------------------------------------------------------------------------------
# Applying a State or an operation to a HIPRenderer
# ---------------------------------------------------------------------------------------------------------------------------
_rows_cache = {}


def scene_arrays(gh, recipe):
    """(rows, data, positions) of a recipe; data / positions (the packed form gsr_set_scene takes) only for raw recipes"""
    key = recipe
    if key not in _rows_cache:
        if len(_rows_cache) >= 16:
            _rows_cache.pop(next(iter(_rows_cache)))
        rows = gh.synth.config_rows(recipe[1]) if recipe[0] == "config" else gh.synth.synth_rows(recipe[1], recipe[2])
        data = pos = None
        if scene_form(recipe) == "raw":
            sc = gh.Scene()
            sc.setData(rows)
            data, pos = sc.data[:8 * sc.vertexCount].copy(), sc.positions
        _rows_cache[key] = (rows, data, pos)
    return _rows_cache[key]


def sh_arrays(gh, spec, n):
    """three half textures of 8 words per splat and the band indices of an SH spec for a scene of n splats"""
    seed, f0, f1, f2 = spec
    rng = np.random.default_rng(seed)
    band = np.array([int(f0 * n) - 1, int(f1 * n) - 1, int(f2 * n) - 1], dtype=np.int32)
    count = n - (int(band[0]) + 1)
    tex = []
    for _ in range(3):
        c = rng.standard_normal((max(count, 0) * 8, 2)) * 0.2
        tex.append(np.ascontiguousarray(gh.pack_half2x16(c[:, 0], c[:, 1]), dtype=np.uint32))
    return tex, band


def camera_of(gh, state, pose=None):
    return gh.orbit_camera(state.pose if pose is None else pose, 120, state.W, state.H, fx=0.59 * state.W)


def _load_scene(gh, r, recipe):
    rows, data, pos = scene_arrays(gh, recipe)
    if scene_form(recipe) == "rows":
        r.set_scene_rows(rows)
    else:
        r.set_raw_scene(data, pos)


def _transform(r, name, values):
    getattr(r, "scene_" + name)(list(values))


def _set_sh(gh, r, spec):
    if spec is None:
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        return
    tex, band = sh_arrays(gh, spec, r._n)
    if r._n - (int(band[0]) + 1) <= 0:      # (no splat carries SH: the call with count 0 clears the state, like None)
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        return
    r.set_sh(tex, band)


def _open_ring(r, ring):
    fmt, full, depth, step = ring
    if depth is None:
        r.open_delivery(3, fmt, full)
    else:
        r.open_delivery_depth(3, fmt, full, (0, 0, 0), depth, step, 0.1)


def build(gh, state, lib_path=None):
    """A context created from the State alone: same kind, same pinned knobs; it has done nothing else."""
    saved = {k: os.environ.get(k) for k, _ in state.knobs}
    try:
        for k, v in state.knobs:
            os.environ[k] = v
        r = gh.HIPRenderer(state.W, state.H, band=state.band, timing=state.timing, throughput=state.kind == "throughput", lib_path=lib_path)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _load_scene(gh, r, state.scene)
    for name, values in state.transforms:
        _transform(r, name, values)
    if state.sh is not None:
        _set_sh(gh, r, state.sh)
    if state.fade != (False, 0.0):
        r.set_depth_fade(*state.fade)
    if state.hit_alpha != 0.5:
        r.set_hit_alpha(state.hit_alpha)
    if state.ring is not None:
        _open_ring(r, state.ring)
    return r


def _frame(gh, r, state, pose=None, sync=False):
    r.set_camera(camera_of(gh, state, pose))
    r.render_async()
    if sync:
        r.sync()


def _refuse(gh, r, state, which):
    """one call the library must refuse; returns the error code it gave"""
    try:
        if which == "band_off_boundary":
            r.set_band(10, 50)
        elif which == "size_zero":
            r.setSize(0, 10)
        elif which == "timing_interval_zero":
            r.set_timing_interval(0)
        else:
            rows = gh.synth.synth_rows(500, 77)
            sc = gh.Scene()
            sc.setData(rows)
            r.set_raw_scene(sc.data[:8 * 500], sc.positions + np.float32(1.0))
    except gh.GsplatError as e:
        return e.code
    raise AssertionError("the library accepted %s" % which)


def apply(gh, r, op, before):
    """Perform `op` on the renderer, which is in State `before`.  Returns a dict of what the operation itself observed
    ({"overflowed": bool} for the overflow operations)."""
    kind, a = op[0], op[1:]
    out = {}
    if kind == "camera":
        _frame(gh, r, before, a[0])                       # (in flight: whatever comes next finds it unsynchronised)
    elif kind == "same_pose":
        for _ in range(2):
            r.set_camera(camera_of(gh, before))
            r._check(r._L.gsr_render(r._ctx))             # the blocking entry point
    elif kind == "burst":
        for p in a:
            _frame(gh, r, before, p)
    elif kind == "sort_only":
        for k in range(a[0]):
            r.sort(camera_of(gh, before, (a[1] + k) % 120))
    elif kind == "readback":
        which = a[0]
        try:
            if which == "records":
                r.read_records()
            elif which == "keys":
                r.read_keys()
            elif which == "bin_lists":
                r.bin_lists()
            elif which == "work_items":
                r.work_items()
            elif which == "depth_index":
                r.lastDepthIndex()
            elif which == "read_depth":
                r.read_depth()
            elif which == "pick":
                r.pick([into_band(before, x, y) for x, y in ((before.W // 2, before.H // 2), (0, 0), (before.W - 1, before.H - 1))])
            else:
                r.stats()
        except gh.GsplatError as e:
            # the one documented refusal: planes and picks of a frame need its bin lists, and the frame enqueued last was sort-only
            # (gsr_sort, or the whole permutation a band context sorts on demand for gsr_read_depth_index / gsr_read_keys)
            assert which in ("read_depth", "pick") and e.code == GSR_ERR_ARG and "sort-only" in str(e), (which, str(e))
    elif kind == "scene":
        _load_scene(gh, r, a[0])
    elif kind == "resize":
        r.setSize(a[0], a[1])
    elif kind == "band":
        r.set_band(a[0], a[1])
    elif kind == "sh":
        _set_sh(gh, r, a[0])
    elif kind in ("limit_box", "rotate", "translate", "scale"):
        _transform(r, kind, a[0])
    elif kind == "fade":
        r.set_depth_fade(a[0], a[1])
    elif kind == "hit_alpha":
        r.set_hit_alpha(a[0])
    elif kind == "depth_async":
        _frame(gh, r, before)
        r.depth_async()                                   # behind the frame, no host wait
        if a[0]:
            r.read_depth()                                # the cached planes; the next frame must not get them
    elif kind == "timing_interval":
        r.set_timing_interval(a[0])
    elif kind == "overflow_sync":
        r.set_list_capacity(a[0])                         # the next frame (the step's own) may not fit: gsr_sync repairs it
    elif kind == "overflow_async":
        r.set_list_capacity(a[0])
        dropped = r.stats()["dropped_frames"]
        for p in a[1:]:
            _frame(gh, r, before, p)
        try:
            r.sync()
            out["overflowed"] = False
        except gh.GsplatError as e:
            assert e.code == GSR_ERR_OVERFLOW, str(e)
            out["overflowed"] = True
        r.sync()                                          # reported once
        assert (r.stats()["dropped_frames"] > dropped) == out["overflowed"]
        assert not r.overflow_pending()
    elif kind == "ring_open":
        _open_ring(r, tuple(a))
    elif kind == "ring_close":
        r.close_delivery()
    elif kind == "deliver":
        _frame(gh, r, before)
        k = r.deliver()
        got = r.acquire(k)
        assert got[0] == k
        r.release(k)
    elif kind == "refused":
        out["code"] = _refuse(gh, r, before, a[0])
    else:
        raise AssertionError(op)
    return out
