// "The value of attribute a of splat i", stated once, beside k_splat_ops.h and by the same rule: every kernel that reduces, bins
// or picks by a splat's own data (k_attr.hip) and the contribution picker (k_contrib_select, k_contrib.hip) call attr_value and
// hold no expression of their own.  The value is an f64, computed in the written order, uncontracted: the units that include this
// are compiled with -ffp-contract=off.  include/gsplat_hip.h ("splat data") has the table the host sees.
#pragma once
#include "gsr_internal.h"
#include "k_splat_ops.h"

namespace gsr {

// the smallest (MAX false) / largest of a splat's three scales; NaN if any of them is
template <bool MAX>
__device__ __forceinline__ double attr_scale_extreme(const float4 s)
{
    const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
    if (x != x || y != y || z != z) return f64_nan();
    double m = x;
    if (MAX ? y > m : y < m) m = y;
    if (MAX ? z > m : z < m) m = z;
    return m;
}

// (a: ATTR_*, valid -- the host refuses every other code; i < n)
__device__ __forceinline__ double attr_value(int a, const AttrSource& s, uint32_t i)
{
    switch (a) {
    case ATTR_X: return (double)s.px[i];
    case ATTR_Y: return (double)s.py[i];
    case ATTR_Z: return (double)s.pz[i];
    case ATTR_DISTANCE: {
        const double dx = (double)s.px[i] - s.ox, dy = (double)s.py[i] - s.oy, dz = (double)s.pz[i] - s.oz;
        return __dsqrt_rn((dx * dx + dy * dy) + dz * dz);   // the correctly rounded square root
    }
    case ATTR_RED: return (double)(s.rgba[i] & 0xffu);
    case ATTR_GREEN: return (double)((s.rgba[i] >> 8) & 0xffu);
    case ATTR_BLUE: return (double)((s.rgba[i] >> 16) & 0xffu);
    case ATTR_OPACITY: return (double)(s.rgba[i] >> 24);
    case ATTR_SCALE_X: return (double)s.scl[i].x;
    case ATTR_SCALE_Y: return (double)s.scl[i].y;
    case ATTR_SCALE_Z: return (double)s.scl[i].z;
    case ATTR_SCALE_MIN: return attr_scale_extreme<false>(s.scl[i]);
    case ATTR_SCALE_MAX: return attr_scale_extreme<true>(s.scl[i]);
    case ATTR_CONTRIB_WEIGHT: return (double)s.weight[i] * (1.0 / 16777216.0);   // "fully opaque pixels' worth"
    case ATTR_CONTRIB_PEAK: return (double)__uint_as_float(s.peak[i]);
    default: return (double)s.pixels[i];                                          // ATTR_CONTRIB_PIXELS
    }
}

}  // namespace gsr
