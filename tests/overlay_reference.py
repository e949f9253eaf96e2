"""What the SELECTION OVERLAY must be ("Selection overlay"; section 5.10), and how far the device's f32 pass
may stray from it: a numpy statement fed by the ORACLE (oracle.project -> rec, bbox, raw; oracle.sort -> the order) and by the
selection as the host holds it, never by device read-backs.  Built on tests/blend_reference.py: its fragments (q in f32,
bit-exact), its exponent a = fma32(q, -log2 e, la), its colours, and the error terms of its Pixels with the same U, E_EXP, E_LA
and SAFETY.

    For a pixel, its fragments are those of the compositor and of "depth and pick": the splats in depth order whose pixel box
    holds it and whose coverage test passes, q <= 4.  From T = 1, S = 0, C = (0, 0, 0), in f64:
        w = T * 2^a;  T -= w;  and if the splat is selected:  S += w;  C += w * c
    cover = S;  delta = mix * (tint * S - C), the overlay minus the framebuffer.

The recurrence IS blend_reference's with a fourth channel of colour 1 (S is the alpha that selected splats supply) and the
colour (0, 0, 0, 0) for a splat that is not selected: an unselected fragment then moves T and eT exactly as there and leaves C,
S and their error terms exactly as they are.  So the bounds of S and C are Pixels' eC, times SAFETY, plus what neither
blend_reference nor the relative u models: results below 2^-126 are rounded to multiples of 2^-149, half of that per operation
and three operations (w, T, the sum) per fragment of the pixel -- 2^-148 per fragment (`kept`).

    bound_S     = SAFETY * eS + kept * 2^-148
    bound_C     = SAFETY * eC + kept * 2^-148
    bound_delta = mix * (|tint| * bound_S + bound_C + u * |tint * S - C|) + u * (|fb| + |delta|)

(the inner fma rounds tint * S - C once; the outer one rounds fb + mix * (...) once, and the comparison subtracts the device's
own fb from the device's overlay, so fb itself carries no error here).

Which pixels have cover > 0.  A pixel without a selected fragment has cover 0 and delta 0 EXACTLY.  One with a selected fragment
has cover > 0 on the device iff one of those fragments' f32 weights is not 0, which can only fail where T * B underflows:
`surely` marks the pixels with a selected fragment of f64 weight >= 2^-126 (minus its bound), `maybe` those with any selected
fragment; the device's set lies between the two, and where the two agree (asserted by the tests of real scenes) it is exact."""
import numpy as np

import blend_reference as BR

_f32, _f64 = np.float32, np.float64
DENORM = 2.0 ** -148
F32_MIN_NORMAL = 2.0 ** -126


class _Overlay(BR.Pixels):
    """blend_reference's recurrence and error terms over four channels: the selected splats' colour sums and S"""

    def __init__(self, h, w, e_exp=BR.E_EXP):
        super().__init__(h, w, e_exp)
        self.C = np.zeros((h, w, 4), _f64)
        self.eC = np.zeros((h, w, 4), _f64)
        self.sel_kept = np.zeros((h, w), np.int32)      # selected fragments of the pixel
        self.sel_wmax = np.zeros((h, w), _f64)          # the largest f64 weight among them, less its bound


def overlay_reference(rec, bbox, raw, order, selected, W, H, window=None, e_exp=BR.E_EXP):
    """The window (x0, y0, w, h) (default: the image) for the selection `selected` (bool[n]) as a dict: S f64[h, w] and its
    bound, C f64[h, w, 3] and its bound, kept / sel_kept i32[h, w] (fragments / selected fragments of the pixel), surely / maybe
    bool[h, w] (see the module's text), T f64[h, w]."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    selected = np.asarray(selected, bool).reshape(-1)
    col = BR.colours(rec, raw)
    px = _Overlay(h, w, e_exp)
    zero = np.zeros(4)
    for i, sl, q in BR.fragments(rec, bbox, order, W, H, window):
        if selected[i]:
            keep = q <= _f32(4.0)
            if keep.any():
                B = np.where(keep, np.exp2(BR.exponent(q, rec[i, 6]).astype(_f64)), 0.0)
                wgt = px.T[sl] * B
                ew = px.eT[sl] * B + wgt * (e_exp + BR.U + BR.LN2 * BR.E_LA * max(1.0, abs(float(rec[i, 6]))))
                px.sel_kept[sl] += keep
                px.sel_wmax[sl] = np.maximum(px.sel_wmax[sl], np.where(keep, wgt - BR.SAFETY * ew, 0.0))
            px.add(sl, q, rec[i, 6], np.concatenate([col[i].astype(_f64), [1.0]]))
        else:
            px.add(sl, q, rec[i, 6], zero)
    floor = px.kept.astype(_f64) * DENORM
    return {"S": px.C[..., 3], "S_bound": BR.SAFETY * px.eC[..., 3] + floor, "C": px.C[..., :3], "C_bound": BR.SAFETY * px.eC[..., :3] + floor[..., None],
            "kept": px.kept, "sel_kept": px.sel_kept, "maybe": px.sel_kept > 0, "surely": px.sel_wmax >= F32_MIN_NORMAL, "T": px.T}


def delta(ref, tint, mix):
    """f64[h, w, 3]: the overlay minus the framebuffer, mix * (tint * S - C)"""
    tint = np.asarray(tint, _f64).reshape(3)
    return float(mix) * (tint[None, None, :] * ref["S"][..., None] - ref["C"])


def delta_bound(ref, tint, mix, fb):
    """f64[h, w, 3]: how far the device's (overlay - fb) may be from delta(); fb: the framebuffer the device added it to, [h, w, >= 3]"""
    tint = np.abs(np.asarray(tint, _f64).reshape(3))
    inner = tint[None, None, :] * ref["S"][..., None] - ref["C"]
    d = float(mix) * inner
    return float(mix) * (tint[None, None, :] * ref["S_bound"][..., None] + ref["C_bound"] + BR.U * np.abs(inner)) + BR.U * (np.abs(np.asarray(fb, _f64)[..., :3]) + np.abs(d))


def compose(fb, ref, tint, mix):
    """f64[h, w, 4]: the overlay the definition gives on top of a framebuffer fb [h, w, 4]"""
    out = np.asarray(fb, _f64).copy()
    out[..., :3] += delta(ref, tint, mix)
    return out


def excess(cover, overlay, fb, ref, tint, mix):
    """(cover, delta): max over the window of |gpu - ref| / bound, at most 1 inside the bounds; pixels without a selected
    fragment are not in it (they are compared exactly)."""
    m = ref["maybe"]
    if not m.any():
        return 0.0, 0.0
    rs = np.abs(np.asarray(cover, _f64) - ref["S"])[m] / ref["S_bound"][m]
    got = np.asarray(overlay, _f64)[..., :3] - np.asarray(fb, _f64)[..., :3]
    rd = np.abs(got - delta(ref, tint, mix))[m] / delta_bound(ref, tint, mix, fb)[m]
    return float(rs.max()), float(rd.max())


def simulate(rec, bbox, raw, order, selected, W, H, fb, tint, mix, window=None, exp_ulps=0, stop_after_last=False):
    """The device's pass in numpy f32: w = T * exp2(a), T = T - w, S = S + w, C = fma(w, c, C) for selected splats, then
    out = fma(mix, fma(tint, S, -C), fb) where the pixel has a non-zero S or C and mix != 0, fb otherwise.  (cover f32[h, w],
    overlay f32[h, w, 4]).  exp_ulps moves a correctly rounded exponential; stop_after_last ends the walk behind the last
    selected splat of the order (the trimmed walk)."""
    x0, y0, w, h = window or (0, 0, W, H)
    rec = np.asarray(rec, _f32).reshape(-1, 8)
    selected = np.asarray(selected, bool).reshape(-1)
    col = BR.colours(rec, raw)
    order = np.asarray(order, np.int64).reshape(-1)
    if stop_after_last:
        hits = np.nonzero(selected[order])[0]
        order = order[:hits[-1] + 1] if hits.size else order[:0]
    T, S = np.ones((h, w), _f32), np.zeros((h, w), _f32)
    C = np.zeros((h, w, 3), _f32)
    for i, sl, q in BR.fragments(rec, bbox, order, W, H, window):
        keep = q <= _f32(4.0)
        if not keep.any():
            continue
        e = np.exp2(BR.exponent(q, rec[i, 6]).astype(_f64)).astype(_f32)
        if exp_ulps:
            e = np.minimum((e.view(np.int32) + np.int32(exp_ulps)).view(_f32), _f32(1.0))
        wgt = np.where(keep, T[sl] * e, _f32(0.0)).astype(_f32)
        T[sl] = T[sl] - wgt
        if selected[i]:
            S[sl] = S[sl] + wgt
            C[sl] = BR._fma(wgt[..., None], col[i][None, None, :], C[sl])
    fb = np.asarray(fb, _f32)
    out = fb.copy()
    if _f32(mix) != 0:
        inner = BR._fma(np.asarray(tint, _f32)[None, None, :], S[..., None], -C)
        new = BR._fma(_f32(mix), inner, fb[..., :3])
        touched = (S != 0) | (C != 0).any(axis=2)
        out[..., :3] = np.where(touched[..., None], new, fb[..., :3])
    return S, out
