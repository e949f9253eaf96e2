// The packed covariance of a splat from its rotation and scale, as Scene.setData / rotate / scale compute it (src/core/Scene.ts:150-176),
// for every kernel that writes cov0..2 (k_scene.hip: the whole scene; k_edit.hip: the selected splats): the arithmetic exists once.
// f64 in the reference's order of operations; the units that include it are compiled with -ffp-contract=off.
#pragma once
#include "gsr_internal.h"

namespace gsr {

// src/utils.ts:16-43 floatToHalf: truncating; JS `>>` takes the shift count modulo 32
__device__ __forceinline__ uint32_t float_to_half_trunc(double value)
{
    const float fv = (float)value;  // _floatView[0] = float
    const int32_t f = __float_as_int(fv);
    const int32_t sign = (f >> 31) & 1;
    const int32_t exp = (f >> 23) & 0xff;
    int32_t frac = f & 0x007fffff;
    int32_t out_exp;
    if (exp == 0) {
        out_exp = 0;
    } else if (exp < 113) {
        out_exp = 0;
        frac = (frac | 0x00800000) >> ((113 - exp) & 31);
        if (frac & 0x01000000) { out_exp = 1; frac = 0; }
    } else if (exp < 142) {
        out_exp = exp - 112;
    } else {
        out_exp = 31;
        frac = 0;
    }
    return (uint32_t)((sign << 15) | (out_exp << 10) | (frac >> 13));
}

__device__ __forceinline__ uint32_t pack_half2(double x, double y)
{
    return float_to_half_trunc(x) | (float_to_half_trunc(y) << 16);
}

// Scene.ts:150-176: rot = (w, x, y, z) as stored in _rotations, scl = _scales.  s[0..5]: the six sums of the covariance
// R^T diag(scale^2) R, entries 00, 01, 02, 11, 12, 22, in front of pack_cov's `4 *` and the halves (k_merge.hip mixes them in f64)
__device__ __forceinline__ void splat_cov(float4 rot, float4 scl, double* s)
{
    const double qx = rot.y, qy = rot.z, qz = rot.w, qw = -(double)rot.x;  // Quaternion(r1, r2, r3, -r0)
    const double R[9] = {1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw,
                         2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw,
                         2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy};
    const double a[9] = {(double)scl.x, 0, 0, 0, (double)scl.y, 0, 0, 0, (double)scl.z};
    const double* b = R;
    // Matrix3.multiply (Matrix3.ts:33-47), this = Diagonal(scale), m = rot
    const double M[9] = {
        b[0] * a[0] + b[3] * a[1] + b[6] * a[2], b[1] * a[0] + b[4] * a[1] + b[7] * a[2], b[2] * a[0] + b[5] * a[1] + b[8] * a[2],
        b[0] * a[3] + b[3] * a[4] + b[6] * a[5], b[1] * a[3] + b[4] * a[4] + b[7] * a[5], b[2] * a[3] + b[5] * a[4] + b[8] * a[5],
        b[0] * a[6] + b[3] * a[7] + b[6] * a[8], b[1] * a[6] + b[4] * a[7] + b[7] * a[8], b[2] * a[6] + b[5] * a[7] + b[8] * a[8]};
    s[0] = M[0] * M[0] + M[3] * M[3] + M[6] * M[6];
    s[1] = M[0] * M[1] + M[3] * M[4] + M[6] * M[7];
    s[2] = M[0] * M[2] + M[3] * M[5] + M[6] * M[8];
    s[3] = M[1] * M[1] + M[4] * M[4] + M[7] * M[7];
    s[4] = M[1] * M[2] + M[4] * M[5] + M[7] * M[8];
    s[5] = M[2] * M[2] + M[5] * M[5] + M[8] * M[8];
}

__device__ __forceinline__ void pack_cov(float4 rot, float4 scl, uint32_t& c0, uint32_t& c1, uint32_t& c2)
{
    double s[6];
    splat_cov(rot, scl, s);
    c0 = pack_half2(4 * s[0], 4 * s[1]);
    c1 = pack_half2(4 * s[2], 4 * s[3]);
    c2 = pack_half2(4 * s[4], 4 * s[5]);
}

}  // namespace gsr
