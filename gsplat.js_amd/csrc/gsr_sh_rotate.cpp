// Rotating SH coefficients (include/gsplat_hip.h, "rotating SH coefficients"; kernel: k_sh_rotate.hip): the
// band matrices of a rotation on the host in f64 (gsr_sh_rotation: pure, no device), the coefficients of the SH rows in scope
// turned in place on the device (gsr_scene_rotate_sh), a selection turned with its coefficients as one edit
// (gsr_scene_rotate_selected_sh), and a frame that is a scaled rotation moved into the coefficients (gsr_scene_bake_sh_frame).
// Every device call is a scene edit ordered like gsr_scene_set_rgba_selected: the context's stream between edit_begin and
// edit_end, every member's frame and sorted order marked as edited.  The SH textures are per-scene state: one call serves every member.
#include "gsr_ctx.h"
#include "k_splat_ops.h"

#include <cmath>
#include <vector>

using namespace gsr;

namespace {

constexpr int SH_SAMPLES = 24;   // Fibonacci-sphere directions of the solve: condition numbers 1.02 / 1.09 / 1.34 for bands 1 / 2 / 3
constexpr int SH_M = 83;         // 9 + 25 + 49

// B_1 .. B_15 at the unit direction d, exactly as eval_sh_channel (k_project.hip) writes the direction factors
void sh_basis(const double* d, double* B)
{
    constexpr double C1 = 0.4886025119029199;
    constexpr double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
    constexpr double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                              1.445305721320277, -0.5900435899266435};
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[0] = -C1 * y; B[1] = -C1 * z; B[2] = C1 * x;
    B[3] = C2[0] * xy; B[4] = C2[1] * yz; B[5] = C2[2] * ((2.0 * zz - xx) - yy); B[6] = C2[3] * xz; B[7] = C2[4] * (xx - yy);
    B[8] = (C3[0] * y) * (3.0 * xx - yy);
    B[9] = (C3[1] * xy) * z;
    B[10] = (C3[2] * y) * ((4.0 * zz - xx) - yy);
    B[11] = (C3[3] * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy);
    B[12] = (C3[4] * x) * ((4.0 * zz - xx) - yy);
    B[13] = (C3[5] * z) * (xx - yy);
    B[14] = (C3[6] * x) * (xx - 3.0 * yy);
}

// D (w x w, row-major) <- the solution of (Y Y^T) D = Y Z^T by Cholesky; Y, Z: w rows of SH_SAMPLES values (the band at S and at R^T S)
void sh_solve_band(int w, const double (*Y)[SH_SAMPLES], const double (*Z)[SH_SAMPLES], double* D)
{
    double A[7][7], L[7][7] = {};
    for (int a = 0; a < w; a++)
        for (int b = 0; b < w; b++) {
            double s = 0.0, t = 0.0;
            for (int i = 0; i < SH_SAMPLES; i++) { s += Y[a][i] * Y[b][i]; t += Y[a][i] * Z[b][i]; }
            A[a][b] = s;
            D[a * w + b] = t;
        }
    for (int a = 0; a < w; a++)
        for (int b = 0; b <= a; b++) {
            double s = A[a][b];
            for (int k = 0; k < b; k++) s -= L[a][k] * L[b][k];
            L[a][b] = a == b ? std::sqrt(s) : s / L[b][b];
        }
    for (int col = 0; col < w; col++) {
        for (int a = 0; a < w; a++) {   // L y = b
            double s = D[a * w + col];
            for (int k = 0; k < a; k++) s -= L[a][k] * D[k * w + col];
            D[a * w + col] = s / L[a][a];
        }
        for (int a = w - 1; a >= 0; a--) {   // L^T x = y
            double s = D[a * w + col];
            for (int k = a + 1; k < w; k++) s -= L[k][a] * D[k * w + col];
            D[a * w + col] = s / L[a][a];
        }
    }
}

// the unit quaternion of q, normalised in f64; false: an entry is not finite, or the length is zero or not finite
bool sh_unit_quaternion(const double* q, double* u)
{
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(q[k])) return false;
    const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (int k = 0; k < 4; k++) u[k] = q[k] / len;
    return true;
}

// m[83] <- D_1, D_2, D_3 of the unit quaternion u
void sh_rotation_of_unit(const double* u, double* m)
{
    for (int k = 0; k < SH_M; k++) m[k] = 0.0;
    if (u[0] == 0.0 && u[1] == 0.0 && u[2] == 0.0) {   // the exact identity
        for (int k = 0; k < 3; k++) m[4 * k] = 1.0;
        for (int k = 0; k < 5; k++) m[9 + 6 * k] = 1.0;
        for (int k = 0; k < 7; k++) m[34 + 8 * k] = 1.0;
        return;
    }
    double R[9];
    quat_matrix(u[0], u[1], u[2], u[3], R);
    static const double golden = M_PI * (1.0 + std::sqrt(5.0));
    double Y[15][SH_SAMPLES], Z[15][SH_SAMPLES];
    for (int i = 0; i < SH_SAMPLES; i++) {
        const double phi = std::acos(1.0 - 2.0 * (i + 0.5) / SH_SAMPLES), theta = golden * (i + 0.5);
        const double d[3] = {std::cos(theta) * std::sin(phi), std::sin(theta) * std::sin(phi), std::cos(phi)};
        double e[3], B[15];   // e = R^T d
        for (int j = 0; j < 3; j++) e[j] = (R[j] * d[0] + R[3 + j] * d[1]) + R[6 + j] * d[2];
        sh_basis(d, B);
        for (int k = 0; k < 15; k++) Y[k][i] = B[k];
        sh_basis(e, B);
        for (int k = 0; k < 15; k++) Z[k][i] = B[k];
    }
    sh_solve_band(3, Y, Z, m);
    sh_solve_band(5, Y + 3, Z + 3, m + 9);
    sh_solve_band(7, Y + 8, Z + 8, m + 34);
}

ShRotation sh_rotation_f32(const double* m)
{
    ShRotation M;
    for (int k = 0; k < 9; k++) M.d1[k] = (float)m[k];
    for (int k = 0; k < 25; k++) M.d2[k] = (float)m[9 + k];
    for (int k = 0; k < 49; k++) M.d3[k] = (float)m[34 + k];
    return M;
}

// the kernel on the rows in scope, between edit_begin and edit_end (the caller has marked the members).  *rows (may be null): the
// rows rotated -- every row is sh_count; the selected ones are counted on the device and copied back, the call's one wait
int sh_rotate_enqueue(gsr_ctx* c, const ShRotation& M, bool selected, uint32_t* rows)
{
    SharedScene& sc = *c->scene;
    if (rows) *rows = 0;
    if (!sc.sh_count || (selected && !sc.sel.mask)) return GSR_OK;
    uint32_t* const tex[3] = {sc.sh_r, sc.sh_g, sc.sh_b};
    const uint32_t first = (uint32_t)(sc.band[0] + 1);
    if (!selected) {
        launch_sh_rotate(sc.n, first, sc.sh_count, tex, nullptr, 0u, M, nullptr, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (rows) *rows = sc.sh_count;
        return GSR_OK;
    }
    constexpr size_t slots = (size_t)SH_ROTATE_COUNTERS * SH_ROTATE_COUNTER_STRIDE;   // the waves' counts, a cache line per slot
    DevBuf<uint32_t> counter;
    if (rows) {
        if (int r = counter.alloc(c, slots)) return r;
        HIP_TRY(c, hipMemsetAsync(counter, 0, slots * 4, c->stream));
    }
    launch_sh_rotate(sc.n, first, sc.sh_count, tex, sc.sel.mask, sc.sel.words, M, counter, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (rows) {
        std::vector<uint32_t> got(slots, 0u);
        HIP_TRY(c, hipMemcpyAsync(got.data(), counter, slots * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < SH_ROTATE_COUNTERS; k++) *rows += got[(size_t)k * SH_ROTATE_COUNTER_STRIDE];
    }
    return GSR_OK;
}

int sh_rotate_scope(gsr_ctx* c, const ShRotation& M, bool selected, uint32_t* rows)
{
    HIP_TRY(c, hipSetDevice(c->device));
    invalidate_members(c, true);   // (a call that would change no bit still counts as an edit)
    if (int r = edit_begin(c)) return r;
    if (int r = sh_rotate_enqueue(c, M, selected, rows)) return r;
    return edit_end(c);
}

}  // namespace

extern "C" {

int gsr_sh_rotation(const double* q, double* m)
{
    if (!q || !m) return fail(nullptr, GSR_ERR_ARG, "gsr_sh_rotation: a NULL pointer");
    double u[4];
    if (!sh_unit_quaternion(q, u)) return fail(nullptr, GSR_ERR_ARG, "gsr_sh_rotation: q = (%g, %g, %g, %g) must be finite and not zero", q[0], q[1], q[2], q[3]);
    sh_rotation_of_unit(u, m);
    return GSR_OK;
}

int gsr_scene_rotate_sh(gsr_ctx* c, const double* q, uint32_t scope, uint32_t* rows)
{
    if (!c || !q) return GSR_ERR_ARG;
    if (scope != GSR_SH_ALL && scope != GSR_SH_SELECTED) return fail(c, GSR_ERR_ARG, "gsr_scene_rotate_sh: unknown scope %u", scope);
    double u[4], m[SH_M];
    if (!sh_unit_quaternion(q, u)) return fail(c, GSR_ERR_ARG, "gsr_scene_rotate_sh: q = (%g, %g, %g, %g) must be finite and not zero", q[0], q[1], q[2], q[3]);
    sh_rotation_of_unit(u, m);
    return sh_rotate_scope(c, sh_rotation_f32(m), scope == GSR_SH_SELECTED, rows);
}

int gsr_scene_rotate_selected_sh(gsr_ctx* c, const double* q, const double* pivot)
{
    if (!c || !q) return GSR_ERR_ARG;
    SharedScene& sc = *c->scene;
    if (!sc.sh_count) return gsr_scene_rotate_selected(c, q, pivot);
    if (int r = require_rows(c)) return r;
    double u[4], m[SH_M];
    if (!sh_unit_quaternion(q, u)) return fail(c, GSR_ERR_ARG, "gsr_scene_rotate_selected_sh: q = (%g, %g, %g, %g) must be finite and not zero", q[0], q[1], q[2], q[3]);
    if (!sc.sh_frame_is_identity())
        return fail(c, GSR_ERR_ARG, "gsr_scene_rotate_selected_sh: the SH frame is not the identity (gsr_scene_bake_sh_frame moves it into the coefficients first)");
    sh_rotation_of_unit(u, m);
    HIP_TRY(c, hipSetDevice(c->device));
    invalidate_members(c, true);
    if (!sc.n || !sc.sel.mask) return GSR_OK;   // never selected in: nothing is launched
    if (int r = edit_begin(c)) return r;
    launch_edit_rotate(sc.n, sc.arr.view(), sc.sel.mask, sc.sel.words, q, pivot, c->stream);   // the geometry: q as given, as gsr_scene_rotate_selected
    HIP_TRY(c, hipGetLastError());
    if (int r = sh_rotate_enqueue(c, sh_rotation_f32(m), true, nullptr)) return r;
    return edit_end(c);
}

int gsr_scene_bake_sh_frame(gsr_ctx* c, double* q_used)
{
    if (!c) return GSR_ERR_ARG;
    SharedScene& sc = *c->scene;
    const double* L = sc.sh_frame;
    if (sc.sh_frame_is_identity()) {
        if (q_used) { q_used[0] = q_used[1] = q_used[2] = 0.0; q_used[3] = 1.0; }
        return GSR_OK;
    }
    // a rotation times a positive uniform scale?  s2: the mean squared row length; G = L L^T / s2 against the identity
    double s2 = 0.0;
    for (int k = 0; k < 9; k++) s2 += L[k] * L[k];
    s2 = s2 / 3.0;
    double worst = std::isfinite(s2) && s2 > 0.0 ? 0.0 : INFINITY;
    for (int i = 0; i < 3 && worst != INFINITY; i++)
        for (int j = 0; j < 3; j++) {
            const double g = (L[3 * i] * L[3 * j] + L[3 * i + 1] * L[3 * j + 1]) + L[3 * i + 2] * L[3 * j + 2];
            const double e = std::fabs(g / s2 - (i == j ? 1.0 : 0.0));
            if (!(e <= worst)) worst = e;   // (a NaN counts as the worst)
        }
    const double det = (L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6])) + L[2] * (L[3] * L[7] - L[4] * L[6]);
    if (!(worst <= 1.0 / 1048576.0) || !(det > 0.0))
        return fail(c, GSR_ERR_ARG, "gsr_scene_bake_sh_frame: the SH frame is not a rotation times a positive uniform scale "
                                    "(L L^T / s2 is %g from the identity, the determinant is %g): it has no rotation to bake", worst, det);
    const double len = std::sqrt(s2);
    double M[12], q[4], t[3], u[4], m[SH_M];   // M = Q^T beside a zero translation, Q = L / sqrt(s2)
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) M[4 * i + j] = L[3 * j + i] / len;
        M[4 * i + 3] = 0.0;
    }
    if (int r = gsr_rigid_decompose(M, q, t)) return fail(c, r, "gsr_scene_bake_sh_frame: the frame's quaternion could not be taken");   // Shepperd's branches
    if (!sh_unit_quaternion(q, u)) return fail(c, GSR_ERR_ARG, "gsr_scene_bake_sh_frame: the frame's quaternion is zero or not finite");
    sh_rotation_of_unit(u, m);
    if (int r = sh_rotate_scope(c, sh_rotation_f32(m), false, nullptr)) return r;
    sc.reset_sh_frame();
    if (q_used) for (int k = 0; k < 4; k++) q_used[k] = q[k];
    return GSR_OK;
}

}  // extern "C"
