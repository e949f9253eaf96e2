"""What a splat's CONTRIBUTION must be ("Contribution"; section 5.8), and how far the device's f32 pass
may stray from it: a numpy statement fed by the ORACLE (oracle.project -> rec, bbox; oracle.sort -> the order), never by
device read-backs.  Built on tests/blend_reference.py: its fragments (q in f32, bit-exact), its exponent
a = fma32(q, -log2 e, la), and the first-order error terms of its Pixels with the same U, E_EXP, E_LA and SAFETY.

    For a pixel, its fragments are those of the compositor and of "depth and pick": the splats in depth order whose pixel
    box holds it and whose coverage test passes, q <= 4.  From T = 1, in f64:  w = T * 2^a;  T -= w.
    Per splat i, over the pixels where i is a fragment (and over the views accumulated):
        pixels[i]  the number of those pixels, exact (coverage is bit-exact: DESIGN 5.5 group A)
        weight[i]  sum of w * 2^24: the device adds rintf(w * 2^24), so its integer lies within
                   sum(SAFETY * ew * 2^24 + 0.5) of it (the 0.5 is the rintf)
        peak[i]    max of w; the device's f32 maximum lies within max(SAFETY * ew) + 2^-24 * peak of it
    with ew the bound of the device's w = T * v_exp_f32(a) as blend_reference derives it:
        ew  = eT * B + T * B * (E_EXP + u + ln 2 * E_LA * max(1, |la|))
    (the depth pass and this one run ONE chain per pixel, so SAFETY = 2, which covers folded segments, is generous here).

simulate() is the device's recurrence in numpy f32 with the integers and the bit-pattern maximum the kernel keeps; its
switches state three wrong passes for the tests of the bounds."""
import numpy as np

import blend_reference as BR

_f32, _f64 = np.float32, np.float64
QUANTA = 2.0 ** 24


class _Walk(BR.Pixels):
    """blend_reference's recurrence and error terms, asked for a fragment's weight and its bound before it is added"""

    def weight(self, sl, q, la):
        """(keep, w, ew) of the fragment on the pixels of sl, from the state in front of it"""
        keep = q <= _f32(4.0)
        B = np.where(keep, np.exp2(BR.exponent(q, la).astype(_f64)), 0.0)
        w = self.T[sl] * B
        ew = self.eT[sl] * B + w * (self.e_exp + BR.U + BR.LN2 * BR.E_LA * max(1.0, abs(float(la))))
        return keep, w, ew


class Contribution:
    """The accumulators of n splats over any number of views, in f64, with their bounds."""

    def __init__(self, n, e_exp=BR.E_EXP):
        self.n, self.e_exp = n, e_exp
        self.pixels = np.zeros(n, np.uint64)
        self.weight = np.zeros(n, _f64)       # quanta of 2^-24
        self.weight_bound = np.zeros(n, _f64)
        self.peak = np.zeros(n, _f64)
        self.peak_err = np.zeros(n, _f64)     # max over the fragments of SAFETY * ew
        self.frames = 0

    def add_view(self, rec, bbox, order, W, H, window=None):
        """one frame: window (x0, y0, w, h) = the pixels that count (default: the image; a band context's columns)"""
        x0, y0, w, h = window or (0, 0, W, H)
        rec = np.asarray(rec, _f32).reshape(-1, 8)
        px = _Walk(h, w, self.e_exp)
        zero = np.zeros(3)
        for i, sl, q in BR.fragments(rec, bbox, order, W, H, window):
            keep, wgt, ew = px.weight(sl, q, rec[i, 6])
            if keep.any():
                self.pixels[i] += np.uint64(keep.sum())
                self.weight[i] += (wgt[keep] * QUANTA).sum()
                self.weight_bound[i] += (BR.SAFETY * ew[keep] * QUANTA + 0.5).sum()
                self.peak[i] = max(self.peak[i], wgt[keep].max())
                self.peak_err[i] = max(self.peak_err[i], BR.SAFETY * ew[keep].max())
            px.add(sl, q, rec[i, 6], zero)
        self.frames += 1
        return self

    def result(self):
        return {"pixels": (self.pixels & np.uint64(0xffffffff)).astype(np.uint32), "weight": self.weight, "weight_bound": self.weight_bound,
                "peak": self.peak, "peak_bound": self.peak_err + 2.0 ** -24 * self.peak, "frames": self.frames}


def contrib_reference(views, n, e_exp=BR.E_EXP):
    """views: [(rec, bbox, order, W, H) or (rec, bbox, order, W, H, window), ...] accumulated; the result dict"""
    c = Contribution(n, e_exp)
    for v in views:
        c.add_view(*v)
    return c.result()


def excess(got, ref):
    """(weight, peak): max over the splats of |got - ref| / bound, at most 1 inside the bounds; got = (weight u64, peak f32, ...)"""
    wr = np.abs(np.asarray(got[0]).astype(_f64) - ref["weight"]) / ref["weight_bound"].clip(min=0.5)
    pr = np.abs(np.asarray(got[1]).astype(_f64) - ref["peak"]) / ref["peak_bound"].clip(min=2.0 ** -149)
    return float(wr.max()) if wr.size else 0.0, float(pr.max()) if pr.size else 0.0


def simulate(rec, bbox, order, W, H, n, window=None, exp_ulps=0, q_max=4.0, no_T=False, peak_sum=False):
    """The device's pass in numpy f32: w = T * exp2(a), T = T - w, per splat the uint64 sum of rint(w * 2^24), the maximum
    of w on its bit patterns and the count of its fragments.  (weight u64[n], peak f32[n], pixels u32[n]).
    exp_ulps moves a correctly rounded exponential; q_max, no_T (w taken as B) and peak_sum (peak accumulated as a sum)
    state wrong passes."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    T = np.ones((h, w), _f32)
    weight, peak, pixels = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    psum = np.zeros(n, _f32)
    for i, sl, q in BR.fragments(rec, bbox, order, W, H, window):
        keep = q <= _f32(q_max)
        if not keep.any():
            continue
        e = np.exp2(BR.exponent(q, rec[i, 6]).astype(_f64)).astype(_f32)
        if exp_ulps:
            e = np.minimum((e.view(np.int32) + np.int32(exp_ulps)).view(_f32), _f32(1.0))
        wgt = np.where(keep, e if no_T else T[sl] * e, _f32(0.0)).astype(_f32)
        T[sl] = T[sl] - wgt
        weight[i] += np.uint64(np.rint(wgt[keep] * _f32(QUANTA)).astype(np.uint64).sum())
        peak[i] = max(peak[i], wgt[keep].view(np.uint32).max())
        psum[i] += wgt[keep].sum(dtype=_f32)
        pixels[i] += np.uint32(keep.sum())
    return weight, (psum if peak_sum else peak.view(_f32)), pixels


def combine(a, b):
    """two passes' (or two ranks') arrays into one: sums add modulo their width, peaks take the maximum"""
    return a[0] + b[0], np.maximum(a[1].view(np.uint32), b[1].view(np.uint32)).view(_f32), a[2] + b[2]


def hidden_stack_scene(length):
    """blend_reference.stack_scene("grey", length) and, behind everything, one small opaque splat at the centre of the frame:
    (camera, splats, index of the hidden splat).  In f32, T reaches EXACTLY 0 only where the stack's B is above 1/2 -- with
    B <= 1/2 it sticks at the smallest denormal, 2^-149 * B rounding to 0 -- which holds under the hidden splat's footprint
    (B = 200 / 255 at the centre) and not at the frame's corners, where the stack's bright splat still gathers 2^-149."""
    cam, splats = BR.stack_scene("grey", length)
    _, to_world = BR.front_view(*BR.STACK_FRAME)
    splats = splats + BR.stack(to_world, 48.0, 48.0, 1, 6.0, (255, 255, 255, 255), dz0=4100 * 1e-3 + 1.0)
    return cam, splats, len(splats) - 1
