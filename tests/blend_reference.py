"""What a pixel's COLOUR must be, and how far the compositor's f32 arithmetic may stray from it: a numpy statement of
DESIGN.md section 5.5, fed by the ORACLE (oracle.project -> rec, bbox, raw; oracle.sort -> the order), never by device
read-backs.  The coverage arithmetic is tests/depth_reference.py's (coverage_q, _fma): it is not restated here.

    For a pixel, its fragments are the splats in depth order whose pixel box holds it and whose coverage test passes:
    q = coverage_q (f32, bit-exact by construction), kept iff q <= 4.  The exponent is ONE f32 fma, reproducible:
        a = fma32(q, -LOG2E32, la)            la = rec[6] = log2(opacity)
    and from there everything is f64:  B = 2^a;  w = T * B;  C += w * c;  T -= w;  alpha = 1 - T   (from T = 1, C = 0).
    The colours c are the ones the kernel uses: (float)byte * (1.0f / 255.0f) in f32 for plain splats, raw[:, 7:10] for
    SH-coloured ones (bit 24 of the record's colour word).

Beside the values runs a first-order bound of the DEVICE's f32 recurrence  w = T * v_exp_f32(a);  T = T - w;
C = fma(w, c, C)  with u = 2^-24 per f32 operation and E_EXP for the relative error of the hardware exponential:

        ew  = eT * B + T * B * (E_EXP + u + ln 2 * E_LA * max(1, |la|))
        eT' = eT * (1 - B) + [the same second term] + min(u * T', w + ew)
        eC' = eC + ew * c + min(u * |C'|, (w + ew) * c)

(the last term of each line is the rounding of that operation's result: half an ulp of it, and never more than the
addend itself -- a sum that returns the old value is off by the addend, which is what happens thousands of times in a
saturated pixel; E_LA: the device's own log2(opacity), see below).  The bound returned is SAFETY * eC + 2^-23 per channel, and likewise for alpha from eT.

Knife edges (a fragment with |q - 4| <= 1e-4 that could still be seen, T * B > 1e-6) are returned as a mask FOR
COMPARISONS WITH THE ORACLE'S MODE 0 ONLY: against this module the kernel's coverage decision is claimed bit-identical
(mode 1), and the GPU tests use no mask."""
import numpy as np

from depth_reference import BIN_PX, coverage_q, _fma

_f32, _f64 = np.float32, np.float64
U = 2.0 ** -24          # one f32 rounding, relative
# Relative error of v_exp_f32 on the arguments the compositor feeds it (-14 < a <= 0).  AMD documents the instruction at
# 1 ulp = 2^-23 relative; E_EXP is twice that.  tests/test_gpu_blend.py (group A) measures it on single-fragment pixels.
E_EXP = 2.0 ** -22
# la = log2(opacity) is the one input of the compositor that is not the oracle's bit for bit: the projection kernel takes it
# with v_log_f32 (documented at 1 ulp), the oracle with log2f (half an ulp), and the record comparison allows 4e-6.  The first GPU
# run of group A found it: single-fragment weights up to 7.1e-7 from 2^a with the ORACLE's la, inside E_EXP with the device's.
# Two ulps of la, |la| >= 1 (an absolute error of a, so a relative one of B after * ln 2):
E_LA = 2.0 ** -22
LN2 = 0.6931471805599453
# The device does not always run the recurrence above front to back in ONE chain: a bin's segments are composited from
# (0, 1) and folded as C0 + T0 * C1, T0 * T1, and k_blend2 does the same with the halves of every 256-entry chunk.  To first
# order a fold adds the same terms in another order plus two roundings per fold: twice the chain's bound covers it.
SAFETY = 2.0
FLOOR = 2.0 ** -23      # the final roundings (alpha = 1 - T in f32, the f32 result itself against an f64 value)
EDGE = 1e-4
EDGE_SEEN = 1e-6
SEEN = 1e-9
LOG2E32 = _f32(1.4426950408889634)
SH_BIT = 1 << 24


def colours(rec, raw):
    """f32[n, 3]: the colour the compositor multiplies a splat's weight with"""
    word = np.ascontiguousarray(np.asarray(rec, _f32).reshape(-1, 8)[:, 7]).view(np.uint32)
    byte = np.stack([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF], axis=1).astype(_f32)
    c = byte * (_f32(1.0) / _f32(255.0))
    sh = (word & SH_BIT) != 0
    c[sh] = np.asarray(raw, _f32).reshape(-1, 12)[sh, 7:10]
    return c


def exponent(q, la):
    """a = fma32(q, -log2(e), la): the argument of the exponential, f32"""
    return _fma(q, -LOG2E32, _f32(la))


def to_rgba8(img):
    """to_rgba8 of gsr_internal.h: uint8(min(max(x, 0), 1) * 255 + 0.5), the product and the sum each rounded to f32"""
    x = np.minimum(np.maximum(np.asarray(img, _f32), _f32(0.0)), _f32(1.0))
    return ((x * _f32(255.0)).astype(_f32) + _f32(0.5)).astype(_f32).astype(np.uint8)


def fragments(rec, bbox, order, W, H, window=None):
    """(splat, slices into the window, q f32[rows, columns]) for every splat of the order whose pixel box meets the window"""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    bb = np.asarray(bbox, np.int64).reshape(-1, 4)
    order = np.asarray(order, np.int64).reshape(-1)
    inside = (bb[:, 0] <= bb[:, 2]) & (bb[:, 1] <= bb[:, 3]) & (bb[:, 2] >= x0) & (bb[:, 0] < x0 + w) & (bb[:, 3] >= y0) & (bb[:, 1] < y0 + h)
    for i in order[inside[order]]:
        xa, xb = max(bb[i, 0], x0), min(bb[i, 2], x0 + w - 1, W - 1)
        ya, yb = max(bb[i, 1], y0), min(bb[i, 3], y0 + h - 1, H - 1)
        if xa > xb or ya > yb:
            continue
        q = coverage_q(rec[i], np.arange(xa, xb + 1), np.arange(ya, yb + 1))
        yield int(i), (slice(ya - y0, yb - y0 + 1), slice(xa - x0, xb - x0 + 1)), q


class Pixels:
    """The f64 recurrence and its f32 error bound over an [h, w] block of pixels; add() takes one fragment per pixel."""

    def __init__(self, h, w, e_exp=E_EXP):
        self.T = np.ones((h, w), _f64)
        self.C = np.zeros((h, w, 3), _f64)
        self.eT = np.zeros((h, w), _f64)
        self.eC = np.zeros((h, w, 3), _f64)
        self.kept = np.zeros((h, w), np.int32)
        self.seen = np.zeros((h, w), np.int32)
        self.mask = np.zeros((h, w), bool)
        self.e_exp = e_exp

    def add(self, sl, q, la, c):
        keep = q <= _f32(4.0)
        edge = np.abs(q.astype(_f64) - 4.0) <= EDGE
        if not (keep.any() or edge.any()):
            return
        B = np.exp2(exponent(q, la).astype(_f64))
        T = self.T[sl]
        self.mask[sl] |= edge & (T * B > EDGE_SEEN)
        B = np.where(keep, B, 0.0)
        c = np.asarray(c, _f64)
        w = T * B
        x = w * (self.e_exp + U + LN2 * E_LA * max(1.0, abs(float(la))))
        ew = self.eT[sl] * B + x
        T1 = T - w
        self.eT[sl] = self.eT[sl] * (1.0 - B) + x + np.minimum(U * T1, w + ew)
        C1 = self.C[sl] + w[..., None] * c
        self.eC[sl] += ew[..., None] * c + np.minimum(U * np.abs(C1), (w + ew)[..., None] * c)
        self.T[sl], self.C[sl] = T1, C1
        self.kept[sl] += keep
        self.seen[sl] += w > SEEN

    def result(self):
        """rgba f64[h, w, 4] (premultiplied, alpha = 1 - T), bound f64[h, w, 4], kept, seen, mask"""
        rgba = np.concatenate([self.C, (1.0 - self.T)[..., None]], axis=2)
        bound = SAFETY * np.concatenate([self.eC, self.eT[..., None]], axis=2) + FLOOR
        return {"rgba": rgba, "bound": bound, "T": self.T, "kept": self.kept, "seen": self.seen, "mask": self.mask}


def blend_reference(rec, bbox, raw, order, W, H, window=None, e_exp=E_EXP):
    """The window (x0, y0, w, h) (default: the image) as a dict: rgba f64[h, w, 4], bound f64[h, w, 4] (how far an f32
    compositor may be from rgba), T f64[h, w], kept / seen i32[h, w] (fragments with q <= 4 / of weight above 1e-9),
    mask bool[h, w] (knife edges: for comparisons with the oracle's mode 0 only)."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    col = colours(rec, raw)
    px = Pixels(h, w, e_exp)
    for i, sl, q in fragments(rec, bbox, order, W, H, window):
        px.add(sl, q, rec[i, 6], col[i])
    return px.result()


def bound_early(ref, eps):
    """The bound of a context with early termination at eps: a tile stops only when every one of its pixels has T < eps, and
    colours are at most 1, so what is missing from any channel is at most eps."""
    return ref["bound"] + eps


def excess(got, ref, bound=None):
    """max over the window of |got - rgba| / bound: at most 1 when the image is inside the bound"""
    b = ref["bound"] if bound is None else bound
    return float((np.abs(np.asarray(got, _f64) - ref["rgba"]) / b).max())


def simulate_f32(rec, bbox, raw, order, W, H, window=None, exp_ulps=0, q_max=4.0, drop=(), rng=None):
    """The device's recurrence in numpy f32 -- w = T * exp2(a), T = T - w, C = fma(w, c, C) -- with a correctly rounded
    exponential moved by exp_ulps ulps (an int, or "random": -1, 0 or +1 per fragment from rng).  q_max and drop state
    wrong compositors for the tests of the bound: another coverage threshold, splats left out.  f32[h, w, 4]."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    col = colours(rec, raw)
    T = np.ones((h, w), _f32)
    C = np.zeros((h, w, 3), _f32)
    for i, sl, q in fragments(rec, bbox, order, W, H, window):
        if i in drop:
            continue
        keep = q <= _f32(q_max)
        if not keep.any():
            continue
        e = np.exp2(exponent(q, rec[i, 6]).astype(_f64)).astype(_f32)
        if isinstance(exp_ulps, str):
            e = (e.view(np.int32) + rng.integers(-1, 2, e.shape).astype(np.int32)).view(_f32)
        elif exp_ulps:
            e = (e.view(np.int32) + np.int32(exp_ulps)).view(_f32)
        wgt = np.where(keep, T[sl] * e, _f32(0.0)).astype(_f32)
        T[sl] = T[sl] - wgt
        C[sl] = _fma(wgt[..., None], col[i][None, None, :], C[sl])
    return np.concatenate([C, (_f32(1.0) - T)[..., None]], axis=2)


def small_quadrant_pairs(rec, bbox, order, W, H, window=None):
    """How many (splat, 8 x 8 quadrant) pairs have the splat covering one to three pixels of the quadrant: the pairs a
    staging mask that is too tight would lose"""
    x0, y0, w, h = window or (0, 0, W, H)
    n = 0
    for i, sl, q in fragments(rec, bbox, order, W, H, window):
        keep = q <= _f32(4.0)
        if not keep.any():
            continue
        ys, xs = np.nonzero(keep)
        quad = ((ys + sl[0].start + y0) // 8) * 65536 + (xs + sl[1].start + x0) // 8
        cnt = np.unique(quad, return_counts=True)[1]
        n += int(((cnt >= 1) & (cnt <= 3)).sum())
    return n


# ---- scenes of tests/test_gpu_blend.py, as lists of dict(pos, scale, rgba, rot) for test_oracle_render.make_scene ----
def _rot_z(theta):
    """rotation about the viewing axis as the four quaternion bytes (w, x, y, z) of a .splat row"""
    b = lambda v: int(np.clip(round(v * 128.0 + 128.0), 0, 255))
    return (b(np.cos(theta / 2)), 128, 128, b(np.sin(theta / 2)))


def front_view(W, H, fx=500.0, z=5.0):
    """(camera, to_world): a camera at (0, 0, -z) looking down +z, and the world position whose centre lands on the pixel
    coordinate (x, y) (row 0 on top) at depth offset dz"""
    from gsplat_hip import Camera
    cam = Camera((0.0, 0.0, -z), (0.0, 0.0, 0.0, 1.0), fx, fx).update(W, H)
    sy = -1.0 if _rows_run_down(cam, W, H) else 1.0

    def to_world(x, y, dz=0.0):
        d = z + dz
        return ((x - W / 2.0) * d / fx, sy * (y - H / 2.0) * d / fx, dz)

    return cam, to_world


def _rows_run_down(cam, W, H):
    """whether +y of the world lands on smaller rows of the image (decided from the camera's own matrices)"""
    v, p, vp = cam.f32()
    clip = np.asarray(vp, _f64).reshape(4, 4).T @ np.array([0.0, 1.0, 0.0, 1.0])
    return clip[1] / clip[3] > 0.0   # positive NDC y is the top of a GL window; rec rows run from the top


def coverage_scene(W, H, regions, seed, per_region=260, giants=False):
    """Group A: isolated or lightly overlapping splats with alpha <= 0.5 and a white or red colour (so that the red channel of
    a single-fragment pixel IS the device's exponential), in `regions` (x0, y0, w, h) of the frame: needles at all angles
    from a pixel to past the 1024-pixel clamp against the thinnest width the projection allows, small splats centred within
    rounding of pixel centres and of quadrant / tile / bin borders, giants over the frame, and splats centred outside a
    region (off screen where the region touches the frame's edge) reaching in by a corner."""
    rng = np.random.default_rng(seed)
    cam, to_world = front_view(W, H)
    thin = 0.0011        # (fx / z)^2 * 4 s^2 just above the 0.3 + sqrt(0.1) the projection needs: the minor axis is a fraction of a pixel
    out = []
    depth = iter(np.linspace(-1.5, 1.5, 200000))
    rgba = lambda: (255, int(rng.choice([0, 255])), int(rng.choice([0, 255])), int(rng.integers(40, 128)))
    for (rx, ry, rw, rh) in regions:
        for k in range(per_region):
            fam = k % 4
            theta = rng.uniform(0.0, np.pi)
            if fam == 0:      # needles: length from a pixel to beyond the clamp
                cx, cy = rx + rng.uniform(0, rw), ry + rng.uniform(0, rh)
                length = float(np.exp(rng.uniform(np.log(0.004), np.log(12.0 if k % 32 == 0 else 0.4))))
                out.append(dict(pos=to_world(cx, cy, next(depth)), scale=(length, thin * rng.uniform(1.0, 1.6), thin), rgba=rgba(), rot=_rot_z(theta)))
            elif fam == 1:    # small splats at pixel centres and at the borders of quadrants, tiles and bins
                step = int(rng.choice([1, 8, 16, 32]))
                gx, gy = rx + step * int(rng.integers(0, max(rw // step, 1) + 1)), ry + step * int(rng.integers(0, max(rh // step, 1) + 1))
                off = 0.5 if step == 1 else float(rng.choice([0.0, 0.5, -0.5]))
                cx, cy = gx + off + rng.choice([0.0, 1e-5, -1e-5, 3e-4, -3e-4]), gy + off + rng.choice([0.0, 1e-5, -1e-5, 3e-4, -3e-4])
                s = thin * float(np.exp(rng.uniform(0.0, np.log(6.0))))
                out.append(dict(pos=to_world(cx, cy, next(depth)), scale=(s * rng.uniform(1.0, 4.0), s, s), rgba=rgba(), rot=_rot_z(theta)))
            elif fam == 2:    # centred outside the region, reaching in by a corner or an edge
                side = int(rng.integers(0, 4))
                r = float(rng.uniform(3.0, 25.0))
                d = r * rng.uniform(0.55, 1.05)
                cx = (rx - d, rx + rw + d, rx + rng.uniform(0, rw), rx - d)[side]
                cy = (ry - d, ry + rh + d, ry - d, ry + rng.uniform(0, rh))[side]
                s = r * 5.0 / 500.0 / (2.0 * np.sqrt(2.0))
                out.append(dict(pos=to_world(cx, cy, next(depth)), scale=(s, s * rng.uniform(0.05, 1.0), s), rgba=rgba(), rot=_rot_z(theta)))
            else:             # needles through the corners of quadrants
                gx, gy = rx + 8 * int(rng.integers(0, rw // 8 + 1)), ry + 8 * int(rng.integers(0, rh // 8 + 1))
                cx, cy = gx + rng.uniform(-1.5, 1.5), gy + rng.uniform(-1.5, 1.5)
                length = float(np.exp(rng.uniform(np.log(0.01), np.log(1.0))))
                out.append(dict(pos=to_world(cx, cy, next(depth)), scale=(length, thin, thin), rgba=rgba(), rot=_rot_z(theta)))
    for k in range(3 if giants else 0):        # giants over the whole frame, faint
        out.append(dict(pos=to_world(W * (0.3 + 0.2 * k), H * (0.6 - 0.1 * k), 2.0 + 0.1 * k), scale=(40.0, 30.0 + 5 * k, 20.0),
                        rgba=(255, 255, 255, 12), rot=_rot_z(0.4 + k)))
    return cam, out


def stack(to_world, x, y, count, radius_px, rgba, dz0=0.0, ddz=1e-3, fx=500.0, z=5.0):
    """count co-located isotropic splats of the given pixel radius, front to back from depth offset dz0"""
    # the axis of an isotropic splat is sqrt(2 * (fx / depth)^2 * 4 s^2) pixels long: s grows with the depth, the footprint stays
    out = []
    for k in range(count):
        s = radius_px * (z + dz0 + ddz * k) / fx / (2.0 * np.sqrt(2.0))
        out.append(dict(pos=to_world(x, y, dz0 + ddz * k), scale=(s, s, s), rgba=rgba))
    return out


# Group D: stacks of co-located splats in front of one bright splat, on a 96 x 96 frame (3 x 3 bins).  Every splat of a wide
# stack enters all nine bins, so each bin's list has exactly len(stack) + 1 entries -- the length of its work item.
STACK_FRAME = (96, 96)
STACK_LENGTHS = (1, 255, 256, 257, 511, 512, 513, 768, 4100)      # of the grey stack
STACK_LENGTH = {"red": 768, "dark": 768, "near": 768, "corner": 4100}


def stack_scene(kind, length):
    """(camera, splats) of one stack; `length` counts the stack AND the bright splat behind it.
    grey:    wide (radius 100 px), opaque-ish: every pixel of the frame saturates within ~60 entries
    red:     the same in pure red: two channels stay zero, so a pixel is finished only at T == 0
    dark:    colour bytes 1 / 255: the saturation threshold 2^-27 * min(R, G, B) lies some 2^-35 below T = 1
    near:    faint splats, then enough opaque ones that T passes 1e-6 (the saturation test's cheap filter) from pixel to pixel
             just in front of the bright splat, then faint ones again
    corner:  the stack ends just short of the corner pixels of the central bin: their quadrants must stay alive, and the
             bright splat behind must appear there"""
    W, H = STACK_FRAME
    cam, to_world = front_view(W, H)
    n = length - 1
    bright = lambda dz: dict(pos=to_world(48.0, 48.0, dz), scale=(1.0, 1.0, 1.0), rgba=(255, 230, 40, 255))
    if kind == "near":
        front = n // 2
        s = stack(to_world, 48.0, 48.0, front, 100.0, (90, 160, 220, 1))
        s += stack(to_world, 48.0, 48.0, 21, 100.0, (200, 150, 100, 128), dz0=1.0)
        s += [bright(1.5)]
        s += stack(to_world, 48.0, 48.0, n - front - 21, 100.0, (90, 160, 220, 1), dz0=2.0)
        return cam, s
    rgba = {"grey": (200, 150, 100, 200), "red": (255, 0, 0, 200), "dark": (1, 1, 1, 200), "corner": (200, 150, 100, 200)}[kind]
    radius = 21.62 if kind == "corner" else 100.0
    return cam, stack(to_world, 48.0, 48.0, n, radius, rgba) + [bright(4100 * 1e-3 + 0.5)]


# Group E: small stacks at the centres of separate bins of a 256 x 96 frame (8 x 3 bins), so that the bins hold exactly these
# many entries: around a chunk, around multiples of both segment lengths, and more than 64 segments' worth.
ITEM_FRAME = (256, 96)
ITEM_COUNTS = (0, 1, 255, 256, 257, 511, 513, 767, 769, 1023, 1025, 64 * 256 + 5)


def item_scene():
    W, H = ITEM_FRAME
    cam, to_world = front_view(W, H)
    rng = np.random.default_rng(77)
    out = []
    for b, count in enumerate(ITEM_COUNTS):
        bx, by = b % 8, b // 8
        out += [dict(pos=to_world(32 * bx + 16.0 + rng.uniform(-2, 2), 32 * by + 16.0 + rng.uniform(-2, 2), -1.0 + 2.0 * k / max(count, 1)),
                     scale=(0.018, 0.018, 0.018), rgba=(int(rng.integers(1, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(1, 40))))
                for k in range(count)]
    return cam, out
