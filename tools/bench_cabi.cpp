// Stand-alone C++ caller of the C ABI (include/gsplat_hip.h): no Python, no Node, no torch.
// SURVEY.md 8(b) lists three callers of libgsplat_hip.so -- the N-API addon, the ctypes harness and a C++ program;
// this is the third.  It renders the bench's 120-pose orbit with F frames in flight and prints one
// JSON line; with --rows / --dump it doubles as a cross-check of the other two hosts (same bytes in, same hashes out).
//
//   bench_cabi [--config C1|C2|C3|C4] [--rows file.splat] [--frames K] [--warmup W] [--in-flight F] [--dump prefix] [--deliver] [--deliver-format nv12|i420] [--deliver-depth f32|u16] [--depth-step 1|2] [--depth-near X] [--depth] [--contrib] [--overlay FRACTION] [--outline WIDTH] [--hide FRACTION] [--hide-edits] [--pick X,Y] [--scene-arrays] [--scene-edit rotate] [--edit-selected FRACTION] [--rotate-sh FRACTION] [--duplicate FRACTION [--reserve]] [--histogram ATTR[:BINS]] [--neighbours RADIUS[:CAP]] [--plane THRESHOLD[:HYPOTHESES]] [--clusters RADIUS[:MIN_PTS]] [--knn RADIUS:K[:kth|mean]] [--normals RADIUS:K[:own]] [--register RADIUS[:ITERATIONS]] [--register-surface RADIUS[:ITERATIONS[:K]]] [--merge CELL] [--share-scene]
// --depth adds legs in which gsr_depth_async is enqueued behind every frame, alternated with plain legs in the same process,
// and reports the frame rate with and without the pass; --pick X,Y prints what gsr_pick returns for that pixel of pose 0.
// --deliver adds a leg in which every frame reaches the host as RGBA8 through the library's delivery ring (gsr_delivery_open,
// gsr_deliver_frame_async, gsr_acquire_frame, gsr_release_frame: three slots per context, the oldest frame picked up when the
// ring is full) -- the header alone is enough to consume frames -- and reports its rate and the checksum of a delivered frame.
// --deliver-format nv12|i420 (beside --deliver) opens the rings in 4:2:0 Y'CbCr instead of RGBA8 (gsr_delivery_open_ex, BT.709 limited
// range, black background) and reports the checksum of the last frame's payload (gsr_delivery_layout gives its size).
// --overlay FRACTION selects that fraction of the splats (scattered over the indices) through gsr_selection_set and adds legs in which
// gsr_overlay_async is enqueued behind every frame, alternated with plain legs as --depth does; then the pass alone on sampled frames
// (overlay_pass_us; with --depth the depth pass on the same frames, depth_pass_us) and the hashes of the overlay's RGBA8 and cover.
// --outline WIDTH (with --overlay) also sets the selection's outline (gsr_set_overlay_outline: white, outer, threshold 0.5), so that
// every overlay pass counted above draws it: overlay_pass_us with and without it is the outline step's cost.
// --contrib adds legs in which gsr_contrib_accumulate_async is enqueued behind every frame, alternated with plain legs as --depth
// does, then times the pass alone on sampled frames (host clock around the enqueue and the wait, the smallest of 20; beside --depth
// the depth pass the same way) and reports `frames` and the FNV-1a of the three accumulator arrays.
// --deliver-depth f32|u16 (beside --deliver) opens depth rings (gsr_delivery_open_depth): every delivered frame carries its hit
// plane, at every --depth-step-th pixel (1, the default, or 2), as float or as 16-bit inverse depth against --depth-near (default
// 0.1), and the checksum of the last frame's plane is reported (gsr_delivery_depth_layout says where it lies in the slot).
//
// --scene-arrays builds every context's scene through gsr_set_scene_arrays instead of gsr_set_scene_rows, from the four arrays
// gsr_read_scene returns for the rows (same scene, same hashes); --scene-edit rotate adds a last leg with a gsr_scene_rotate by one
// degree about y in front of every frame (a turntable: the scene is edited on the device, nothing is uploaded) and reports its rate.
// --share-scene: with --in-flight k, contexts 2..k call gsr_share_scene(ctx, first) instead of uploading: one device copy of the
// scene for all of them.  The report carries scene_sharing (members, bytes held once) and setup_ms, the wall time from the first
// gsr_create to the last scene being ready, with and without the flag.
// --hide FRACTION hides that fraction of the splats (scattered over the indices) through gsr_hidden_set on every device copy before
// the first frame, so every timed frame is one of the scene with those out of the way; the report carries `hidden` and the call's
// wall time.  --hide 0 is the run to compare with: nothing hidden, the projection handed no mask.  --hide-edits adds, at the very
// end, the wall time of one gsr_hide_selected and of one gsr_scene_erase_selected with and without a hidden set to carry along.
// --edit-selected FRACTION selects that fraction of the splats (scattered over the indices) through gsr_selection_set on every device
// copy and adds a leg with a gsr_scene_rotate_selected by one degree about y, pivoted, behind every frame: only the selection turns.
// The report carries the leg's rate and `edit_ms`, the wall time a frame of that leg takes beyond a frame of the plain timed loop.
// --rotate-sh FRACTION, after the frame legs: gives every splat an SH row (seeded halves; bandsIndices -1, n / 3, 2n / 3), selects
// that fraction of the splats (scattered over the indices) and reports the blocking time (the call and gsr_sync, the median of five)
// of gsr_scene_rotate_sh over every row, of gsr_scene_rotate_sh over the selected rows with its count, and of
// gsr_scene_rotate_selected_sh (the selected splats turned about a pivot with their coefficients), with the rows rotated.
// --histogram ATTR[:BINS] (x, y, z, distance, red, green, blue, opacity, scale_x .. scale_max, contrib_weight .. contrib_pixels; 256
// bins unless given; the contribution attributes go beside --contrib) asks the scene about itself: gsr_attr_stats, a
// gsr_attr_histogram over [min, max] and a gsr_select_attr of the middle half of the bins, [edge(bins / 4), edge(bins - bins / 4)).
// The report carries the three blocking times (the best of five each) and the check sum(counts[a .. b-1]) == selected.
// --neighbours RADIUS[:CAP] (cap 64 unless given) counts every splat's neighbours within RADIUS: five gsr_neighbours calls, the best
// wall time, and by the library's events on the stream the index build (with its bound) and the count pass apart; pair_bound and
// the pair tests per second it means for the count pass, the median count, the splats with fewer than three neighbours, and the
// check that gsr_select_neighbours(lo 0, hi 3) selects exactly hist[0] + hist[1] + hist[2].
// --plane THRESHOLD[:HYPOTHESES] (512 hypotheses unless given) fits the scene's dominant plane: five gsr_fit_plane calls, the best
// wall time, and by the library's events on the stream the candidate pass and the scoring pass apart; the tests and the tests per
// second they mean for the scoring pass, the winner's inliers, and the check that gsr_select_plane(plane, -THRESHOLD, THRESHOLD)
// selects exactly that many splats (`fit_equals_selection`).
// --clusters RADIUS[:MIN_PTS] (min_pts 0 unless given) labels the islands of the scene at the linking radius: five gsr_clusters calls,
// the best wall time, and by the library's events on the stream the stages apart -- the index with its bound, the core test with the
// seed, union with flatten, border with sizes; clusters, largest_size and noise, and the check that gsr_select_clusters(0, 10)
// selects exactly the splats whose sizes[i] is below 10 (`sizes_equal_selection`).
// --knn RADIUS:K[:kth|mean] (mean unless given) finds every splat's K nearest neighbours within RADIUS: five gsr_knn calls without
// the lists and five with them, the best wall time of either, and by the library's events on the stream the index build (with its
// bound) and the walk (with its fill) apart; pair_bound and the pair tests per second it means for the walk, complete,
// finite_values, the value range, and the check that gsr_select_knn(lo = the mean of the finite values, hi = +inf) selects exactly
// the splats whose values[i] is at or above it (`values_equal_selection`).
// --normals RADIUS:K[:own] computes every splat's surface normal: five gsr_normals calls from the K nearest neighbours within RADIUS
// (with `own`: from the splat's own shortest axis, RADIUS and K unread), the best blocking time, and by the library's events on the
// stream the index build (with its bound; 0 for own) and the walk (with its fill; own: the one kernel) apart; pair_bound, valid, the
// variation range, and the check that gsr_select_normal(variation, lo = 0, hi = the mean of the valid variations) selects exactly the
// splats whose variation[i] lies in that closed range (`variation_equals_selection`).
// --register RADIUS[:ITERATIONS] (32 steps at most unless given) registers the scene to a copy of itself: a second context holds the
// config's scene moved by a fixed small rigid motion (0.01 rad about (0.3, 0.9, 0.2), then (0.01, -0.005, 0.008)), so source and target
// are one size; one gsr_register call from the identity at tolerance 2^-40: its blocking time, the status, every step's pairs and rms,
// and by the library's events on the stream the target's index (built once per call) and, of the last step and summed over the
// steps, the bound, the walk and the tree apart (gsr_debug_match_times).
// --register-surface RADIUS[:ITERATIONS[:K]] runs gsr_register_surface on --register's moved copy (made for either option): the
// target's own normals without K, KNN normals with k = K at RADIUS; one call from the identity at tolerance 2^-40: its blocking
// time, the status, every step's pairs, surface_pairs and both rms, and by the library's events the target's normals (index with
// its bound, and walk or own kernel: gsr_debug_normals_times on the target), the target's index, and of the last step and summed
// over the steps the bound, the walk and the rows + tree stage apart.  With --register in the same run the walk and the bound are
// the same kernels on the same data, and the 16-wide rows + tree stage is the new stage's yardstick.
// --merge CELL (behind everything else: it replaces the scene) merges the cells of a grid of side CELL: three gsr_cells calls, the
// best wall time of the report, then the one gsr_scene_merge_cells call it announced: the blocking time, the rows before and after,
// the members per cell, and the check that the edit left the announced rows with exactly the merged rows selected (`report_equals_edit`).
// --duplicate FRACTION (last of all: it grows the scene) selects that fraction of the splats through gsr_selection_set and calls
// gsr_scene_duplicate_selected twice -- the second call copies the first one's copies, the same count -- and reports the wall time
// of either (`duplicate_ms`, `duplicate_again_ms`), the count and the capacity.  With --reserve, gsr_scene_reserve makes room for
// both first (`reserve_ms`), so neither call re-allocates the scene arrays or copies an old row.
//
// Scene: the seeded synthetic generator of gsplat_hip/synth.py (mulberry32 counter PRNG, 24 draws per splat) written
// out again in C++; log/exp/cos come from libm here and from numpy there, so a byte may differ in a rare rounding --
// pass --rows to feed the exact bytes another host used.  Scene.setData itself runs on the device (gsr_set_scene_rows).
// Camera: Camera.update (src/cameras/Camera.ts:81-92) and the OrbitControls pose formula (OrbitControls.ts:275-283)
// in double precision, rounded to float like `new Float32Array(m.buffer)`.
// Build: gsplat.js_amd/csrc/Makefile (target bench_cabi), plain g++ against the header and the shared library.
#include "../include/gsplat_hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Config { const char* name; uint32_t seed, n; int w, h; double sigma, s_lo, s_hi, fx; };
const Config CONFIGS[] = {
    {"C1", 1, 10000, 640, 480, 1.5, 0.004, 0.06, 1132.0},
    {"C2", 2, 300000, 1920, 1080, 1.0, 0.003, 0.04, 1132.0},
    {"C3", 3, 1000000, 1920, 1080, 1.5, 0.004, 0.06, 1132.0},
    {"C4", 4, 5000000, 3840, 2160, 1.5, 0.004, 0.06, 2264.0},
};

uint32_t mulberry32(uint32_t seed, uint64_t call)   // call is 1-based, like synth.mulberry32
{
    uint32_t t = (uint32_t)(seed + call * 0x6D2B79F5ull);
    t = (t ^ (t >> 15)) * (t | 1u);
    t = t ^ (t + (t ^ (t >> 7)) * (t | 61u));
    return t ^ (t >> 14);
}

std::vector<uint8_t> synth_rows(const Config& c)
{
    const int DRAWS = 24;
    std::vector<uint8_t> out((size_t)c.n * 32);
    const double ls = std::log(c.s_lo), lr = std::log(c.s_hi) - std::log(c.s_lo);
    for (uint32_t i = 0; i < c.n; i++) {
        double u[DRAWS];
        for (int d = 0; d < DRAWS; d++) u[d] = (double)mulberry32(c.seed, (uint64_t)i * DRAWS + d + 1) / 4294967296.0;
        auto normal = [&](int a, int b) { return std::sqrt(-2.0 * std::log(1.0 - u[a])) * std::cos(2.0 * M_PI * u[b]); };
        uint8_t* row = &out[(size_t)i * 32];
        for (int k = 0; k < 3; k++) {
            double p = normal(2 * k, 2 * k + 1) * c.sigma;
            p = p < -6.0 ? -6.0 : p > 6.0 ? 6.0 : p;
            const float pf = (float)p, sf = (float)std::exp(ls + u[6 + k] * lr);
            std::memcpy(row + 4 * k, &pf, 4);
            std::memcpy(row + 12 + 4 * k, &sf, 4);
            row[24 + k] = (uint8_t)std::floor(256.0 * u[9 + k]);
        }
        row[27] = (uint8_t)(32 + std::floor(224.0 * u[12]));
        double q[4], len = 0;
        for (int k = 0; k < 4; k++) { q[k] = normal(13 + 2 * k, 14 + 2 * k); len += q[k] * q[k]; }
        len = std::sqrt(len);
        if (len < 1e-12) len = 1e-12;
        for (int k = 0; k < 4; k++) {
            double v = std::nearbyint(q[k] / len * 128.0 + 128.0);   // numpy.round: half to even
            row[28 + k] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
    }
    return out;
}

struct Cam { float view[16], proj[16], vp[16]; };

Cam orbit_camera(int k, int frames, int W, int H, double fx)
{
    const double alpha = 2.0 * M_PI * k / frames, beta = 0.3, radius = 8.0, near = 0.01, far = 1000.0;
    const double x = radius * std::sin(alpha) * std::cos(beta), y = -radius * std::sin(beta), z = -radius * std::cos(alpha) * std::cos(beta);
    double dx = -x, dy = -y, dz = -z;
    const double ln = std::sqrt(dx * dx + dy * dy + dz * dz);
    dx /= ln; dy /= ln; dz /= ln;
    const double rx = std::asin(-dy), ry = std::atan2(dx, dz);
    // Quaternion.FromEuler (src/math/Quaternion.ts:65-83) with ez = 0
    const double hx = rx / 2, hy = ry / 2, cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hx), sp = std::sin(hx), cz = 1.0, sz = 0.0;
    const double qx = cy * sp * cz + sy * cp * sz, qy = sy * cp * cz - cy * sp * sz, qz = cy * cp * sz - sy * sp * cz,
                 qw = cy * cp * cz + sy * sp * sz;
    // Matrix3.RotationFromQuaternion (src/math/Matrix3.ts:67-80)
    const double R[9] = {1 - 2 * qy * qy - 2 * qz * qz, 2 * qx * qy - 2 * qz * qw, 2 * qx * qz + 2 * qy * qw,
                         2 * qx * qy + 2 * qz * qw, 1 - 2 * qx * qx - 2 * qz * qz, 2 * qy * qz - 2 * qx * qw,
                         2 * qx * qz - 2 * qy * qw, 2 * qy * qz + 2 * qx * qw, 1 - 2 * qx * qx - 2 * qy * qy};
    const double P[16] = {2 * fx / W, 0, 0, 0, 0, -2 * fx / H, 0, 0, 0, 0, far / (far - near), 1, 0, 0, -(far * near) / (far - near), 0};
    const double V[16] = {R[0], R[1], R[2], 0, R[3], R[4], R[5], 0, R[6], R[7], R[8], 0,
                          -x * R[0] - y * R[3] - z * R[6], -x * R[1] - y * R[4] - z * R[7], -x * R[2] - y * R[5] - z * R[8], 1};
    Cam c;
    for (int i = 0; i < 4; i++)      // Matrix4.multiply (src/math/Matrix4.ts:32-53): viewProj = projection.multiply(view)
        for (int j = 0; j < 4; j++)
            c.vp[4 * i + j] = (float)(V[4 * i + 0] * P[j] + V[4 * i + 1] * P[4 + j] + V[4 * i + 2] * P[8 + j] + V[4 * i + 3] * P[12 + j]);
    for (int i = 0; i < 16; i++) { c.view[i] = (float)V[i]; c.proj[i] = (float)P[i]; }
    return c;
}

uint64_t fnv1a(const void* p, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

extern "C" int gsr_debug_neighbour_times(gsr_ctx* ctx, float* out /* build_ms, count_ms */);   // not part of the ABI (gsr_neighbours.cpp)
extern "C" int gsr_debug_plane_times(gsr_ctx* ctx, float* out /* candidates_ms, score_ms */);   // not part of the ABI (gsr_plane.cpp)
extern "C" int gsr_debug_knn_times(gsr_ctx* ctx, float* out /* index_ms, walk_ms */);   // not part of the ABI (gsr_knn.cpp)
extern "C" int gsr_debug_normals_times(gsr_ctx* ctx, float* out /* index_ms, walk_ms */);   // not part of the ABI (gsr_normals.cpp)
extern "C" int gsr_debug_match_times(gsr_ctx* ctx, float* out /* index_ms, the last step's bound_ms, walk_ms, tree_ms, the steps' sums of the three, steps */);   // not part of the ABI (gsr_match.cpp)
extern "C" int gsr_debug_cluster_times(gsr_ctx* ctx, float* out /* index_ms, core_ms, union_ms, border_ms */);   // not part of the ABI (gsr_clusters.cpp)

#define CHECK(call)                                                                                     \
    do {                                                                                                \
        const int rc_ = (call);                                                                         \
        if (rc_) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, gsr_last_error(ctx0)); return 1; } \
    } while (0)

}  // namespace

int main(int argc, char** argv)
{
    std::string config = "C1", rows_path, dump;
    int frames = 240, warmup = 20, in_flight = 3;
    bool deliver = false;
    std::string deliver_format = "rgba8";
    std::string deliver_depth = "none";
    int depth_step = 1;
    float depth_near = 0.1f;
    bool contrib = false;
    double overlay_fraction = -1.0;   // < 0: off
    int outline_width = 0;            // 0: off
    bool depth = false, pick = false, scene_arrays = false, share_scene = false;
    std::string scene_edit = "none";
    double hide_fraction = -1.0;   // < 0: off
    bool hide_edits = false;
    double edit_fraction = -1.0;   // < 0: off
    double rotate_sh_fraction = -1.0;   // < 0: off
    double duplicate_fraction = -1.0;   // < 0: off
    bool reserve = false;
    std::string histogram_attr;         // empty: off
    uint32_t histogram_bins = 256;
    double nb_radius = 0.0;             // 0: off
    uint32_t nb_cap = 64;
    double plane_threshold = -1.0;      // < 0: off
    uint32_t plane_hypotheses = 512;
    double cl_radius = 0.0;             // 0: off
    uint32_t cl_min_pts = 0;
    double knn_radius = 0.0;            // 0: off
    double merge_cell = 0.0;            // 0: off
    double reg_radius = 0.0;            // 0: off
    uint32_t reg_steps = 32;
    double rs_radius = 0.0;             // --register-surface; 0: off
    uint32_t rs_steps = 32, rs_k = 0;   // rs_k 0: the target's own normals
    uint32_t knn_k = 8;
    int32_t knn_stat = GSR_KNN_MEAN;
    double normals_radius = 0.0;        // 0: off
    uint32_t normals_k = 8;
    bool normals_own = false;
    int32_t pick_xy[2] = {0, 0};
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--config") config = next();
        else if (a == "--rows") rows_path = next();
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--warmup") warmup = std::atoi(next());
        else if (a == "--in-flight") in_flight = std::atoi(next());
        else if (a == "--dump") dump = next();
        else if (a == "--deliver") deliver = true;
        else if (a == "--deliver-format") deliver_format = next();
        else if (a == "--deliver-depth") deliver_depth = next();
        else if (a == "--depth-step") depth_step = std::atoi(next());
        else if (a == "--depth-near") depth_near = (float)std::atof(next());
        else if (a == "--depth") depth = true;
        else if (a == "--contrib") contrib = true;
        else if (a == "--outline" && i + 1 < argc) { outline_width = std::atoi(argv[++i]); if (outline_width < 1 || outline_width > 16) { std::fprintf(stderr, "--outline WIDTH must be in 1 .. 16\n"); return 2; } }
        else if (a == "--overlay" && i + 1 < argc) { overlay_fraction = std::atof(argv[++i]); if (!(overlay_fraction >= 0.0 && overlay_fraction <= 1.0)) { std::fprintf(stderr, "--overlay FRACTION must be in [0, 1]\n"); return 2; } }
        else if (a == "--hide" && i + 1 < argc) { hide_fraction = std::atof(argv[++i]); if (!(hide_fraction >= 0.0 && hide_fraction <= 1.0)) { std::fprintf(stderr, "--hide FRACTION must be in [0, 1]\n"); return 2; } }
        else if (a == "--hide-edits") hide_edits = true;
        else if (a == "--rotate-sh" && i + 1 < argc) { rotate_sh_fraction = std::atof(argv[++i]); if (!(rotate_sh_fraction >= 0.0 && rotate_sh_fraction <= 1.0)) { std::fprintf(stderr, "--rotate-sh FRACTION must be in [0, 1]\n"); return 2; } }
        else if (a == "--edit-selected" && i + 1 < argc) { edit_fraction = std::atof(argv[++i]); if (!(edit_fraction >= 0.0 && edit_fraction <= 1.0)) { std::fprintf(stderr, "--edit-selected FRACTION must be in [0, 1]\n"); return 2; } }
        else if (a == "--histogram" && i + 1 < argc) {
            histogram_attr = argv[++i];
            const size_t colon = histogram_attr.find(':');
            if (colon != std::string::npos) { histogram_bins = (uint32_t)std::atoi(histogram_attr.c_str() + colon + 1); histogram_attr.resize(colon); }
            if (histogram_bins < 1 || histogram_bins > 4096) { std::fprintf(stderr, "--histogram ATTR[:BINS]: BINS must be in 1 .. 4096\n"); return 2; }
        }
        else if (a == "--neighbours" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':');
            nb_radius = std::atof(v.c_str());
            if (colon != std::string::npos) nb_cap = (uint32_t)std::atoi(v.c_str() + colon + 1);
            if (!(nb_radius > 0.0) || nb_cap < 1 || nb_cap > GSR_NEIGHBOUR_MAX_CAP) { std::fprintf(stderr, "--neighbours RADIUS[:CAP]: RADIUS > 0, CAP in 1 .. 4095\n"); return 2; }
        }
        else if (a == "--plane" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':');
            plane_threshold = std::atof(v.c_str());
            if (colon != std::string::npos) plane_hypotheses = (uint32_t)std::atoi(v.c_str() + colon + 1);
            if (!(plane_threshold >= 0.0) || plane_hypotheses < 1 || plane_hypotheses > GSR_PLANE_MAX_HYPOTHESES) { std::fprintf(stderr, "--plane THRESHOLD[:HYPOTHESES]: THRESHOLD >= 0, HYPOTHESES in 1 .. 4096\n"); return 2; }
        }
        else if (a == "--clusters" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':');
            cl_radius = std::atof(v.c_str());
            int mp = colon != std::string::npos ? std::atoi(v.c_str() + colon + 1) : 0;
            if (!(cl_radius > 0.0) || mp < 0 || mp > (int)GSR_NEIGHBOUR_MAX_CAP) { std::fprintf(stderr, "--clusters RADIUS[:MIN_PTS]: RADIUS > 0, MIN_PTS in 0 .. 4095\n"); return 2; }
            cl_min_pts = (uint32_t)mp;
        }
        else if (a == "--knn" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':'), colon2 = colon == std::string::npos ? colon : v.find(':', colon + 1);
            knn_radius = std::atof(v.c_str());
            const int k = colon != std::string::npos ? std::atoi(v.c_str() + colon + 1) : 0;
            const std::string stat = colon2 != std::string::npos ? v.substr(colon2 + 1) : "mean";
            if (!(knn_radius > 0.0) || k < 1 || k > (int)GSR_KNN_MAX_K || (stat != "kth" && stat != "mean")) { std::fprintf(stderr, "--knn RADIUS:K[:kth|mean]: RADIUS > 0, K in 1 .. 32\n"); return 2; }
            knn_k = (uint32_t)k; knn_stat = stat == "kth" ? GSR_KNN_KTH : GSR_KNN_MEAN;
        }
        else if (a == "--normals" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':'), colon2 = colon == std::string::npos ? colon : v.find(':', colon + 1);
            normals_radius = std::atof(v.c_str());
            const int k = colon != std::string::npos ? std::atoi(v.c_str() + colon + 1) : 0;
            const std::string source = colon2 != std::string::npos ? v.substr(colon2 + 1) : "knn";
            if (!(normals_radius > 0.0) || k < 2 || k > (int)GSR_KNN_MAX_K || (source != "own" && source != "knn")) { std::fprintf(stderr, "--normals RADIUS:K[:own]: RADIUS > 0, K in 2 .. 32\n"); return 2; }
            normals_k = (uint32_t)k; normals_own = source == "own";
        }
        else if (a == "--register" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':');
            reg_radius = std::atof(v.c_str());
            const int steps = colon != std::string::npos ? std::atoi(v.c_str() + colon + 1) : 32;
            if (!(reg_radius > 0.0) || steps < 1 || steps > (int)GSR_REGISTER_MAX_ITERATIONS_LIMIT) { std::fprintf(stderr, "--register RADIUS[:ITERATIONS]: RADIUS > 0, ITERATIONS in 1 .. 256\n"); return 2; }
            reg_steps = (uint32_t)steps;
        }
        else if (a == "--register-surface" && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t colon = v.find(':'), colon2 = colon == std::string::npos ? colon : v.find(':', colon + 1);
            rs_radius = std::atof(v.c_str());
            const int steps = colon != std::string::npos ? std::atoi(v.c_str() + colon + 1) : 32;
            const int k = colon2 != std::string::npos ? std::atoi(v.c_str() + colon2 + 1) : 0;
            if (!(rs_radius > 0.0) || steps < 1 || steps > (int)GSR_REGISTER_MAX_ITERATIONS_LIMIT || (colon2 != std::string::npos && (k < 2 || k > (int)GSR_KNN_MAX_K))) {
                std::fprintf(stderr, "--register-surface RADIUS[:ITERATIONS[:K]]: RADIUS > 0, ITERATIONS in 1 .. 256, K in 2 .. 32\n"); return 2;
            }
            rs_steps = (uint32_t)steps; rs_k = (uint32_t)k;
        }
        else if (a == "--merge" && i + 1 < argc) { merge_cell = std::atof(argv[++i]); if (!(merge_cell > 0.0)) { std::fprintf(stderr, "--merge CELL: CELL > 0\n"); return 2; } }
        else if (a == "--duplicate" && i + 1 < argc) { duplicate_fraction = std::atof(argv[++i]); if (!(duplicate_fraction >= 0.0 && duplicate_fraction <= 1.0)) { std::fprintf(stderr, "--duplicate FRACTION must be in [0, 1]\n"); return 2; } }
        else if (a == "--reserve") reserve = true;
        else if (a == "--scene-arrays") scene_arrays = true;
        else if (a == "--scene-edit") scene_edit = next();
        else if (a == "--share-scene") share_scene = true;
        else if (a == "--pick") { pick = std::sscanf(next(), "%d,%d", &pick_xy[0], &pick_xy[1]) == 2; if (!pick) { std::fprintf(stderr, "--pick X,Y\n"); return 2; } }
        else { std::fprintf(stderr, "usage: bench_cabi [--config C1..C4] [--rows f.splat] [--frames K] [--warmup W] [--in-flight F] [--dump prefix] [--deliver] [--deliver-format nv12|i420] [--deliver-depth f32|u16] [--depth-step 1|2] [--depth-near X] [--depth] [--contrib] [--overlay FRACTION] [--outline WIDTH] [--hide FRACTION] [--hide-edits] [--pick X,Y] [--scene-arrays] [--scene-edit rotate] [--edit-selected FRACTION] [--rotate-sh FRACTION] [--duplicate FRACTION [--reserve]] [--histogram ATTR[:BINS]] [--neighbours RADIUS[:CAP]] [--plane THRESHOLD[:HYPOTHESES]] [--clusters RADIUS[:MIN_PTS]] [--knn RADIUS:K[:kth|mean]] [--normals RADIUS:K[:own]] [--register RADIUS[:ITERATIONS]] [--register-surface RADIUS[:ITERATIONS[:K]]] [--merge CELL] [--share-scene]\n"); return 2; }
    }
    const Config* cfg = nullptr;
    for (const Config& c : CONFIGS) if (config == c.name) cfg = &c;
    if (!cfg || in_flight < 1 || frames < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const int32_t format = deliver_format == "nv12" ? GSR_FORMAT_NV12 : deliver_format == "i420" ? GSR_FORMAT_I420 : GSR_FORMAT_RGBA8;
    if (format == GSR_FORMAT_RGBA8 && deliver_format != "rgba8") { std::fprintf(stderr, "--deliver-format nv12|i420\n"); return 2; }
    const int32_t depth_format = deliver_depth == "f32" ? GSR_DEPTH_F32 : deliver_depth == "u16" ? GSR_DEPTH_U16 : GSR_DEPTH_NONE;
    if (depth_format == GSR_DEPTH_NONE && deliver_depth != "none") { std::fprintf(stderr, "--deliver-depth f32|u16\n"); return 2; }
    if (scene_edit != "none" && scene_edit != "rotate") { std::fprintf(stderr, "--scene-edit rotate\n"); return 2; }
    if (depth_format != GSR_DEPTH_NONE && !deliver) { std::fprintf(stderr, "--deliver-depth goes beside --deliver\n"); return 2; }
    if (outline_width && overlay_fraction < 0.0) { std::fprintf(stderr, "--outline WIDTH goes beside --overlay FRACTION\n"); return 2; }

    std::vector<uint8_t> rows;
    if (!rows_path.empty()) {
        FILE* f = std::fopen(rows_path.c_str(), "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", rows_path.c_str()); return 2; }
        std::fseek(f, 0, SEEK_END);
        rows.resize((size_t)std::ftell(f));
        std::fseek(f, 0, SEEK_SET);
        if (std::fread(rows.data(), 1, rows.size(), f) != rows.size()) { std::fclose(f); return 2; }
        std::fclose(f);
    } else {
        rows = synth_rows(*cfg);
    }
    const uint32_t n = (uint32_t)(rows.size() / 32);

    gsr_ctx* ctx0 = nullptr;
    std::vector<gsr_ctx*> ctx(in_flight, nullptr);
    const auto setup0 = std::chrono::steady_clock::now();
    for (int c = 0; c < in_flight; c++) {
        gsr_options o{};
        o.device = 0; o.width = cfg->w; o.height = cfg->h;
        o.flags = in_flight > 1 ? GSR_FLAG_THROUGHPUT : 0;
        const int rc = gsr_create(&ctx[c], &o);
        if (rc) { std::fprintf(stderr, "gsr_create failed (%d): %s\n", rc, gsr_last_error(nullptr)); return 1; }
        ctx0 = ctx[c];
        if (share_scene && c > 0) CHECK(gsr_share_scene(ctx[c], ctx[0]));
        else CHECK(gsr_set_scene_rows(ctx[c], rows.data(), n));
    }
    if (scene_arrays) {   // the same scene once more, as a host that holds a Scene's four arrays hands it over
        std::vector<uint32_t> data((size_t)n * 8);
        std::vector<float> positions((size_t)n * 3), rotations((size_t)n * 4), scales((size_t)n * 3);
        ctx0 = ctx[0];
        CHECK(gsr_read_scene(ctx[0], data.data(), positions.data(), rotations.data(), scales.data(), nullptr));
        for (gsr_ctx* c : ctx) {
            ctx0 = c;
            if (share_scene && c != ctx[0]) CHECK(gsr_share_scene(c, ctx[0]));
            else CHECK(gsr_set_scene_arrays(c, data.data(), positions.data(), rotations.data(), scales.data(), n));
        }
    }
    const double setup_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - setup0).count() * 1e3;
    int32_t share_members = 0;
    uint64_t share_bytes = 0;
    ctx0 = ctx[in_flight - 1];
    CHECK(gsr_scene_sharing(ctx[in_flight - 1], &share_members, &share_bytes));
    std::vector<Cam> poses(120);
    for (int k = 0; k < 120; k++) poses[k] = orbit_camera(k, 120, cfg->w, cfg->h, cfg->fx);
    // --hide: a seeded fraction of the splats (scattered over the indices, the hash --overlay uses, another seed) is hidden on every
    // device copy before any frame is enqueued: every frame below, warm-up included, is a frame of the scene with those out of the way
    uint32_t hidden = 0;
    double hidden_set_ms = 0;
    if (hide_fraction >= 0.0) {
        std::vector<uint32_t> words((n + 31) / 32, 0u);
        const uint64_t limit = (uint64_t)(hide_fraction * 4294967296.0);
        for (uint32_t i = 0; i < n; i++)
            if ((uint64_t)((i + 0x9e3779b9u) * 2654435761u) < limit) words[i >> 5] |= 1u << (i & 31);
        const auto h0 = std::chrono::steady_clock::now();
        ctx0 = ctx[0];
        CHECK(gsr_hidden_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, &hidden));
        hidden_set_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - h0).count() * 1e3;
        if (!share_scene) for (gsr_ctx* c : ctx) { ctx0 = c; if (c != ctx[0]) CHECK(gsr_hidden_set(c, words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr)); }
    }

    auto step = [&](int k) -> int {
        gsr_ctx* c = ctx[k % in_flight];
        const Cam& p = poses[k % 120];
        if (int rc = gsr_set_camera(c, p.view, p.proj, p.vp, (float)cfg->fx, (float)cfg->fx)) return rc;
        return gsr_render_async(c);
    };
    for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(step(k)); }
    for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(step(warmup + k)); }
    for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // one more frame at pose 0 on context 0 for the cross-check hashes
    ctx0 = ctx[0];
    CHECK(gsr_set_camera(ctx[0], poses[0].view, poses[0].proj, poses[0].vp, (float)cfg->fx, (float)cfg->fx));
    CHECK(gsr_render(ctx[0]));
    std::vector<uint32_t> di(n);
    std::vector<uint8_t> px((size_t)cfg->w * cfg->h * 4);
    CHECK(gsr_read_depth_index(ctx[0], di.data()));
    CHECK(gsr_read_pixels_rgba8(ctx[0], px.data()));
    if (!dump.empty()) {
        FILE* f = std::fopen((dump + ".depth_index.bin").c_str(), "wb");
        if (f) { std::fwrite(di.data(), 4, di.size(), f); std::fclose(f); }
        f = std::fopen((dump + ".rgba8.bin").c_str(), "wb");
        if (f) { std::fwrite(px.data(), 1, px.size(), f); std::fclose(f); }
    }
    // --depth: the orbit again, three legs without and three with the depth pass behind every frame, alternating
    double depth_sec[2] = {0, 0};
    if (depth) {
        for (int leg = 0; leg < 6; leg++) {
            const bool with = leg & 1;
            auto depth_step = [&](int k) -> int {
                if (int rc = step(k)) return rc;
                return with ? gsr_depth_async(ctx[k % in_flight]) : 0;
            };
            for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(depth_step(k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            const auto d0 = std::chrono::steady_clock::now();
            for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(depth_step(warmup + k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            depth_sec[with] += std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        }
    }
    // --contrib: the orbit again, three legs without and three with the contribution pass (gsr_contrib_accumulate_async) behind
    // every frame, alternating; then the pass alone on a sampled frame of context 0 (and, with --depth, the depth pass on the same
    // frame): the stream is drained, the pass enqueued and waited for, so the figure holds one launch's latency as well
    double contrib_sec[2] = {0, 0}, contrib_pass_ms = 0, depth_pass_ms = 0;
    uint32_t contrib_frames = 0;
    unsigned long long contrib_hash[3] = {0, 0, 0};
    if (contrib) {
        ctx0 = ctx[0];
        CHECK(gsr_contrib_reset(ctx[0]));
        if (!share_scene) for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_contrib_reset(c)); }
        for (int leg = 0; leg < 6; leg++) {
            const bool with = leg & 1;
            auto contrib_step = [&](int k) -> int {
                if (int rc = step(k)) return rc;
                return with ? gsr_contrib_accumulate_async(ctx[k % in_flight]) : 0;
            };
            for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(contrib_step(k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            const auto d0 = std::chrono::steady_clock::now();
            for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(contrib_step(warmup + k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            contrib_sec[with] += std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        }
        ctx0 = ctx[0];
        const int samples = 20;
        for (int pass = 0; pass < (depth ? 2 : 1); pass++) {
            double best = 1e30;
            for (int k = 0; k < samples; k++) {
                const Cam& p = poses[(7 * k) % 120];
                CHECK(gsr_set_camera(ctx[0], p.view, p.proj, p.vp, (float)cfg->fx, (float)cfg->fx));
                CHECK(gsr_render(ctx[0]));
                const auto p0 = std::chrono::steady_clock::now();
                CHECK(pass ? gsr_depth_async(ctx[0]) : gsr_contrib_accumulate_async(ctx[0]));
                CHECK(gsr_sync(ctx[0]));
                best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - p0).count() * 1e3);
            }
            (pass ? depth_pass_ms : contrib_pass_ms) = best;
        }
        std::vector<uint64_t> cw(n);
        std::vector<float> cp(n);
        std::vector<uint32_t> cx(n);
        CHECK(gsr_read_contrib(ctx[0], cw.data(), cp.data(), cx.data(), n, &contrib_frames));
        contrib_hash[0] = fnv1a(cw.data(), (size_t)n * 8); contrib_hash[1] = fnv1a(cp.data(), (size_t)n * 4); contrib_hash[2] = fnv1a(cx.data(), (size_t)n * 4);
    }
    // --overlay: the orbit again, three legs without and three with the overlay pass (gsr_overlay_async) behind every frame,
    // alternating; then the pass alone on sampled frames of context 0, measured as --contrib measures its pass
    double overlay_sec[2] = {0, 0}, overlay_pass_us = 0, overlay_depth_pass_us = 0;
    uint32_t overlay_selected = 0;
    unsigned long long overlay_hash[2] = {0, 0};
    if (overlay_fraction >= 0.0) {
        ctx0 = ctx[0];
        std::vector<uint32_t> words((n + 31) / 32, 0u);
        const uint64_t limit = (uint64_t)(overlay_fraction * 4294967296.0);
        for (uint32_t i = 0; i < n; i++)
            if ((uint64_t)(i * 2654435761u) < limit) words[i >> 5] |= 1u << (i & 31);
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, &overlay_selected));
        if (!share_scene) for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_selection_set(c, words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr)); }
        gsr_overlay_options oo{};
        oo.tint[0] = 1.0f; oo.tint[1] = 0.5f; oo.tint[2] = 0.0f; oo.mix = 0.5f;
        for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_set_overlay(c, &oo)); }
        if (outline_width) {   // the selection's outline behind every overlay pass: the legs, the pass and the hashes below include it
            gsr_outline_options ol{};
            ol.rgb[0] = ol.rgb[1] = ol.rgb[2] = 1.0f; ol.alpha = 1.0f; ol.threshold = 0.5f; ol.width = outline_width; ol.side = GSR_OUTLINE_OUTER;
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_set_overlay_outline(c, &ol)); }
        }
        for (int leg = 0; leg < 6; leg++) {
            const bool with = leg & 1;
            auto overlay_step = [&](int k) -> int {
                if (int rc = step(k)) return rc;
                return with ? gsr_overlay_async(ctx[k % in_flight]) : 0;
            };
            for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(overlay_step(k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            const auto d0 = std::chrono::steady_clock::now();
            for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(overlay_step(warmup + k)); }
            for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
            overlay_sec[with] += std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        }
        ctx0 = ctx[0];
        const int samples = 20;
        for (int pass = 0; pass < (depth ? 2 : 1); pass++) {
            double best = 1e30;
            for (int k = 0; k < samples; k++) {
                const Cam& p = poses[(7 * k) % 120];
                CHECK(gsr_set_camera(ctx[0], p.view, p.proj, p.vp, (float)cfg->fx, (float)cfg->fx));
                CHECK(gsr_render(ctx[0]));
                const auto p0 = std::chrono::steady_clock::now();
                CHECK(pass ? gsr_depth_async(ctx[0]) : gsr_overlay_async(ctx[0]));
                CHECK(gsr_sync(ctx[0]));
                best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - p0).count() * 1e6);
            }
            (pass ? overlay_depth_pass_us : overlay_pass_us) = best;
        }
        CHECK(gsr_set_camera(ctx[0], poses[0].view, poses[0].proj, poses[0].vp, (float)cfg->fx, (float)cfg->fx));
        CHECK(gsr_render(ctx[0]));
        std::vector<uint8_t> o8((size_t)cfg->w * cfg->h * 4);
        std::vector<float> cov((size_t)cfg->w * cfg->h);
        CHECK(gsr_read_overlay_rgba8(ctx[0], o8.data()));
        CHECK(gsr_read_overlay(ctx[0], nullptr, cov.data()));
        overlay_hash[0] = fnv1a(o8.data(), o8.size()); overlay_hash[1] = fnv1a(cov.data(), cov.size() * 4);
    }
    gsr_pick_result picked{};
    if (pick) {
        ctx0 = ctx[0];
        CHECK(gsr_set_camera(ctx[0], poses[0].view, poses[0].proj, poses[0].vp, (float)cfg->fx, (float)cfg->fx));
        CHECK(gsr_render(ctx[0]));
        CHECK(gsr_pick(ctx[0], pick_xy, 1, &picked));
    }
    // --deliver: the same orbit with every frame delivered; then pose 0 once more, delivered, against the blocking read above
    double delivered_sec = 0;
    unsigned long long delivered_hash = 0, delivered_depth_hash = 0;
    gsr_depth_layout dlay{};
    uint64_t delivered = 0, sink = 0;
    if (deliver) {
        for (gsr_ctx* c : ctx) {
            ctx0 = c;
            if (format == GSR_FORMAT_RGBA8 && depth_format == GSR_DEPTH_NONE) { CHECK(gsr_delivery_open(c, 3)); continue; }
            gsr_delivery_options dopt{};
            dopt.slots = 3; dopt.format = format;
            if (depth_format == GSR_DEPTH_NONE) { CHECK(gsr_delivery_open_ex(c, &dopt)); continue; }
            gsr_depth_delivery_options ddopt{};
            ddopt.format = depth_format; ddopt.step = depth_step; ddopt.near = depth_near;
            CHECK(gsr_delivery_open_depth(c, &dopt, &ddopt));
        }
        auto pick_up = [&](gsr_ctx* c) -> int {   // the oldest frame of this context
            gsr_frame f;
            if (int rc = gsr_acquire_frame(c, 0, &f)) return rc;
            sink += f.pixels[(size_t)f.width * f.height / 2];
            if (depth_format != GSR_DEPTH_NONE) sink += f.pixels[dlay.offset + dlay.bytes / 2];
            delivered++;
            return gsr_release_frame(c, f.serial);
        };
        if (depth_format != GSR_DEPTH_NONE) CHECK(gsr_delivery_depth_layout(ctx[0], &dlay));   // (every context's: same size, same options)
        auto deliver_step = [&](int k) -> int {
            gsr_ctx* c = ctx[k % in_flight];
            if (int rc = step(k)) return rc;
            int rc = gsr_deliver_frame_async(c, nullptr);
            if (rc == GSR_ERR_BUSY) {
                if ((rc = pick_up(c))) return rc;
                rc = gsr_deliver_frame_async(c, nullptr);
            }
            return rc;
        };
        auto drain = [&]() -> int {
            for (gsr_ctx* c : ctx)
                while (gsr_frame_ready(c, 0) >= 0) { ctx0 = c; if (int rc = pick_up(c)) return rc; }
            return 0;
        };
        for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(deliver_step(k)); }
        CHECK(drain());
        delivered = 0;
        const auto d0 = std::chrono::steady_clock::now();
        for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(deliver_step(warmup + k)); }
        CHECK(drain());
        delivered_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        if (delivered != (uint64_t)frames) { std::fprintf(stderr, "%llu of %d frames were delivered\n", (unsigned long long)delivered, frames); return 1; }
        ctx0 = ctx[0];
        CHECK(gsr_set_camera(ctx[0], poses[0].view, poses[0].proj, poses[0].vp, (float)cfg->fx, (float)cfg->fx));
        CHECK(gsr_render_async(ctx[0]));
        uint64_t serial = 0;
        gsr_frame f;
        CHECK(gsr_deliver_frame_async(ctx[0], &serial));
        CHECK(gsr_acquire_frame(ctx[0], serial, &f));
        gsr_frame_layout lay;
        CHECK(gsr_delivery_layout(ctx[0], &lay));
        delivered_hash = (unsigned long long)fnv1a(f.pixels, (size_t)lay.bytes);
        // (a Y'CbCr payload is held to the definition by tests/test_gpu_yuv_delivery.py, through this checksum)
        // (and the depth plane by tests/test_gpu_depth_delivery.py, through this one)
        if (depth_format != GSR_DEPTH_NONE) delivered_depth_hash = (unsigned long long)fnv1a(f.pixels + dlay.offset, (size_t)dlay.bytes);
        const bool same = f.width == cfg->w && f.height == cfg->h && lay.format == format &&
                          (format != GSR_FORMAT_RGBA8 || (lay.bytes == px.size() && !std::memcmp(f.pixels, px.data(), px.size())));
        CHECK(gsr_release_frame(ctx[0], serial));
        if (!same) { std::fprintf(stderr, "the delivered frame differs from gsr_read_pixels_rgba8\n"); return 1; }
    }
    // --scene-edit rotate: the orbit once more with the scene turned on the device in front of every frame (last: it changes the scene)
    double edit_sec = 0;
    if (scene_edit == "rotate") {
        const double half = 0.5 * 3.14159265358979323846 / 180.0, dq[4] = {0.0, std::sin(half), 0.0, std::cos(half)};
        auto edit_step = [&](int k) -> int {
            if (int rc = gsr_scene_rotate(ctx[k % in_flight], dq)) return rc;
            return step(k);
        };
        for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(edit_step(k)); }
        for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
        const auto e0 = std::chrono::steady_clock::now();
        for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(edit_step(warmup + k)); }
        for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
        edit_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - e0).count();
    }
    // --edit-selected: the orbit once more with the selected splats turned about a pivot on the device behind every frame
    double edit_selected_sec = 0;
    uint32_t edit_selected = 0;
    if (edit_fraction >= 0.0) {
        std::vector<uint32_t> words((n + 31) / 32, 0u);
        const uint64_t limit = (uint64_t)(edit_fraction * 4294967296.0);
        for (uint32_t i = 0; i < n; i++)
            if ((uint64_t)((i + 0x85ebca6bu) * 2654435761u) < limit) words[i >> 5] |= 1u << (i & 31);
        for (gsr_ctx* c : ctx) {   // (the members of a shared scene have one selection: the first call sets it)
            ctx0 = c;
            if (c == ctx[0] || !share_scene) CHECK(gsr_selection_set(c, words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, &edit_selected));
        }
        const double half = 0.5 * 3.14159265358979323846 / 180.0, dq[4] = {0.0, std::sin(half), 0.0, std::cos(half)}, pivot[3] = {0.5, 0.0, -0.5};
        auto edit_step = [&](int k) -> int {
            if (int rc = step(k)) return rc;
            return gsr_scene_rotate_selected(ctx[k % in_flight], dq, pivot);
        };
        for (int k = 0; k < warmup; k++) { ctx0 = ctx[k % in_flight]; CHECK(edit_step(k)); }
        for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
        const auto e0 = std::chrono::steady_clock::now();
        for (int k = 0; k < frames; k++) { ctx0 = ctx[(warmup + k) % in_flight]; CHECK(edit_step(warmup + k)); }
        for (gsr_ctx* c : ctx) { ctx0 = c; CHECK(gsr_sync(c)); }
        edit_selected_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - e0).count();
    }
    // --rotate-sh: the SH rows rotated on the device; behind the frame legs, which render the scene without SH
    double rotate_sh_all_ms = 0, rotate_sh_selected_ms = 0, rotate_selected_sh_ms = 0;
    uint32_t rotate_sh_rows_all = 0, rotate_sh_rows = 0;
    if (rotate_sh_fraction >= 0.0) {
        ctx0 = ctx[0];
        {
            std::vector<uint32_t> tex[3];
            uint32_t state = 0x9e3779b9u;
            for (auto& t : tex) {
                t.resize((size_t)n * 8);
                for (uint32_t& w : t) {   // two halves in (-1, 1): sign, exponent 8 .. 14, any mantissa
                    state = state * 1664525u + 1013904223u;
                    const uint32_t lo = (state >> 8) & 0xffffu, hi = (state >> 16) ^ (state & 0xffffu);
                    auto half = [](uint32_t v) { return (v & 0x83ffu) | ((8u + ((v >> 10) & 31u) % 7u) << 10); };
                    w = half(lo) | (half(hi) << 16);
                }
            }
            const int32_t band[3] = {-1, (int32_t)(n / 3), (int32_t)(2 * (n / 3))};
            CHECK(gsr_set_scene_sh(ctx[0], tex[0].data(), tex[1].data(), tex[2].data(), n, band));
        }
        std::vector<uint32_t> words((n + 31) / 32, 0u);
        const uint64_t limit = (uint64_t)(rotate_sh_fraction * 4294967296.0);
        for (uint32_t i = 0; i < n; i++)
            if ((uint64_t)((i + 0x85ebca6bu) * 2654435761u) < limit) words[i >> 5] |= 1u << (i & 31);
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr));
        const double half = 0.5 * 3.14159265358979323846 / 180.0, dq[4] = {0.0, std::sin(half), 0.0, std::cos(half)}, pivot[3] = {0.5, 0.0, -0.5};
        auto median_ms = [&](auto call, double* out) -> int {
            double t[5];
            for (double& v : t) {
                if (int rc = gsr_sync(ctx[0])) return rc;
                const auto t0 = std::chrono::steady_clock::now();
                if (int rc = call()) return rc;
                if (int rc = gsr_sync(ctx[0])) return rc;
                v = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
            }
            std::sort(t, t + 5);
            *out = t[2];
            return 0;
        };
        CHECK(median_ms([&] { return gsr_scene_rotate_sh(ctx[0], dq, GSR_SH_ALL, &rotate_sh_rows_all); }, &rotate_sh_all_ms));
        CHECK(median_ms([&] { return gsr_scene_rotate_sh(ctx[0], dq, GSR_SH_SELECTED, &rotate_sh_rows); }, &rotate_sh_selected_ms));
        CHECK(median_ms([&] { return gsr_scene_rotate_selected_sh(ctx[0], dq, pivot); }, &rotate_selected_sh_ms));
    }
    // --hide-edits (last: it removes splats): the wall time of one gsr_hide_selected that hides a fifth of the scene, and of one
    // gsr_scene_erase_selected of another fifth while those are hidden (the compaction carries the hidden set: k_box_compact_bits)
    double hide_selected_ms = 0, erase_hidden_ms = 0, erase_plain_ms = 0;
    uint32_t edits_hidden = 0, edits_kept = 0;
    if (hide_edits) {
        ctx0 = ctx[0];
        std::vector<uint32_t> words((n + 31) / 32, 0u);
        auto fifth = [&](uint32_t r) { std::fill(words.begin(), words.end(), 0u); for (uint32_t i = 0; i < n; i++) if (i % 5u == r) words[i >> 5] |= 1u << (i & 31); };
        auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count() * 1e3; };
        CHECK(gsr_hidden_set(ctx[0], nullptr, 0, GSR_SELOP_REPLACE, nullptr));
        fifth(0);
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr));
        auto t = std::chrono::steady_clock::now();
        CHECK(gsr_scene_erase_selected(ctx[0], 0, nullptr));                       // nothing hidden: the compaction as it was
        erase_plain_ms = ms_since(t);
        fifth(1);
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr));
        t = std::chrono::steady_clock::now();
        CHECK(gsr_hide_selected(ctx[0], GSR_SELOP_ADD, &edits_hidden));
        hide_selected_ms = ms_since(t);
        fifth(2);
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, nullptr));
        t = std::chrono::steady_clock::now();
        CHECK(gsr_scene_erase_selected(ctx[0], 0, &edits_kept));                   // with the hidden set carried through
        erase_hidden_ms = ms_since(t);
        CHECK(gsr_read_hidden(ctx[0], nullptr, 0, &edits_hidden));
    }
    // --histogram: the scene asked about itself -- statistics, a histogram over [min, max], the middle half of its bins selected
    int32_t hist_attr = -1;
    uint32_t hist_count = 0, hist_nan = 0, hist_outside[3] = {0, 0, 0}, hist_selected = 0, hist_a = 0, hist_b = 0;
    unsigned long long hist_sum = 0, hist_peak = 0;
    double hist_min = 0, hist_max = 0, hist_lo = 0, hist_hi = 1, hist_ms[3] = {0, 0, 0};
    if (!histogram_attr.empty()) {
        static const char* const ATTR_NAMES[16] = {"x", "y", "z", "distance", "red", "green", "blue", "opacity", "scale_x", "scale_y", "scale_z",
                                                   "scale_min", "scale_max", "contrib_weight", "contrib_peak", "contrib_pixels"};   // GSR_ATTR_*
        for (int k = 0; k < 16; k++) if (histogram_attr == ATTR_NAMES[k]) hist_attr = k;
        if (hist_attr < 0) { std::fprintf(stderr, "--histogram: unknown attribute %s\n", histogram_attr.c_str()); return 2; }
        const double origin[3] = {0.0, 0.0, 0.0};
        const uint32_t bins = histogram_bins;
        std::vector<uint32_t> counts(bins);
        auto best_of = [&](auto call, double& ms) -> int {
            ms = 1e30;
            for (int t = 0; t < 5; t++) {
                const auto t0 = std::chrono::steady_clock::now();
                if (int rc = call()) return rc;
                ms = std::min(ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
            }
            return 0;
        };
        ctx0 = ctx[0];
        CHECK(best_of([&] { return gsr_attr_stats(ctx[0], hist_attr, origin, 0, &hist_count, &hist_nan, &hist_min, &hist_max); }, hist_ms[0]));
        if (std::isfinite(hist_min) && std::isfinite(hist_max)) { hist_lo = hist_min; hist_hi = std::nextafter(hist_max, INFINITY); }   // the maximum is in range
        CHECK(best_of([&] { return gsr_attr_histogram(ctx[0], hist_attr, origin, 0, hist_lo, hist_hi, bins, counts.data(), hist_outside); }, hist_ms[1]));
        // the edges, by the header's f64 rule
        const double w = (hist_hi - hist_lo) / (double)bins;
        auto edge = [&](uint32_t k) { return k == bins ? hist_hi : std::min(hist_lo + (double)k * w, hist_hi); };
        hist_a = bins / 4; hist_b = bins - bins / 4;
        CHECK(best_of([&] { return gsr_select_attr(ctx[0], hist_attr, origin, edge(hist_a), edge(hist_b), GSR_SELOP_REPLACE, &hist_selected); }, hist_ms[2]));
        for (uint32_t k = 0; k < bins; k++) { hist_peak = std::max<unsigned long long>(hist_peak, counts[k]); if (k >= hist_a && k < hist_b) hist_sum += counts[k]; }
    }
    // --neighbours: every splat's neighbour count within the radius, the stages timed apart, the floater pick checked against the histogram
    gsr_neighbour_info nb_info{};
    double nb_ms = 1e30, nb_build_ms = 1e30, nb_count_ms = 1e30, nb_select_ms = 0;
    uint32_t nb_median = 0, nb_selected = 0, nb_n = 0;
    unsigned long long nb_few = 0;
    if (nb_radius > 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &nb_n));
        std::vector<uint32_t> counts(nb_n), hist(nb_cap + 1u);
        for (int t = 0; t < 5; t++) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_neighbours(ctx[0], nb_radius, nb_cap, 0, 0, counts.data(), nb_n, hist.data(), &nb_info));
            nb_ms = std::min(nb_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
            float stage[2] = {0, 0};
            CHECK(gsr_debug_neighbour_times(ctx[0], stage));
            nb_build_ms = std::min(nb_build_ms, (double)stage[0]); nb_count_ms = std::min(nb_count_ms, (double)stage[1]);
        }
        unsigned long long seen = 0;
        for (uint32_t k = 0; k <= nb_cap; k++) { seen += hist[k]; if (2 * seen >= nb_info.in_scope) { nb_median = k; break; } }
        for (uint32_t k = 0; k < 3 && k <= nb_cap; k++) nb_few += hist[k];
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(gsr_select_neighbours(ctx[0], nb_radius, nb_cap, 0, 0, 0, std::min(3u, nb_cap + 1u), GSR_SELOP_REPLACE, &nb_selected, nullptr));
        nb_select_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    }
    // --plane: the dominant plane, the stages timed apart, the winner's score checked against the picker
    gsr_plane_info pl_info{};
    double pl_ms = 1e30, pl_cand_ms = 1e30, pl_score_ms = 1e30, pl_select_ms = 0;
    uint32_t pl_selected = 0;
    if (plane_threshold >= 0.0) {
        ctx0 = ctx[0];
        for (int t = 0; t < 5; t++) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_fit_plane(ctx[0], plane_threshold, plane_hypotheses, 0, 0, 0, nullptr, &pl_info));
            pl_ms = std::min(pl_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
            float stage[2] = {0, 0};
            CHECK(gsr_debug_plane_times(ctx[0], stage));
            pl_cand_ms = std::min(pl_cand_ms, (double)stage[0]); pl_score_ms = std::min(pl_score_ms, (double)stage[1]);
        }
        if (pl_info.found) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_select_plane(ctx[0], pl_info.plane, -plane_threshold, plane_threshold, GSR_SELOP_REPLACE, &pl_selected));
            pl_select_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
        }
    }
    // --clusters: the islands at the linking radius, the stages timed apart, the small-island pick checked against the sizes
    gsr_cluster_info cl_info{};
    double cl_ms = 1e30, cl_stage_ms[4] = {1e30, 1e30, 1e30, 1e30}, cl_select_ms = 0;
    uint32_t cl_selected = 0, cl_n = 0;
    unsigned long long cl_small = 0;
    if (cl_radius > 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &cl_n));
        std::vector<uint32_t> labels(cl_n), sizes(cl_n);
        for (int t = 0; t < 5; t++) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_clusters(ctx[0], cl_radius, cl_min_pts, 0, 0, labels.data(), sizes.data(), cl_n, &cl_info));
            cl_ms = std::min(cl_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
            float stage[4] = {0, 0, 0, 0};
            CHECK(gsr_debug_cluster_times(ctx[0], stage));
            for (int k = 0; k < 4; k++) cl_stage_ms[k] = std::min(cl_stage_ms[k], (double)stage[k]);
        }
        for (uint32_t i = 0; i < cl_n; i++) cl_small += sizes[i] < 10u;
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(gsr_select_clusters(ctx[0], cl_radius, cl_min_pts, 0, 0, 0, 10, GSR_SELOP_REPLACE, &cl_selected, nullptr));
        cl_select_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    }
    // --knn: every splat's k nearest within the radius, without and with the lists, the stages timed apart, the pick checked against the values
    gsr_knn_info knn_info{};
    double knn_ms[2] = {1e30, 1e30}, knn_index_ms[2] = {1e30, 1e30}, knn_walk_ms[2] = {1e30, 1e30}, knn_select_ms = 0, knn_lo = 0;
    uint32_t knn_selected = 0, knn_n = 0;
    unsigned long long knn_above = 0;
    if (knn_radius > 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &knn_n));
        std::vector<uint32_t> found(knn_n), idx((size_t)knn_n * knn_k), hist(knn_k + 1u);
        std::vector<double> d2((size_t)knn_n * knn_k), values(knn_n);
        for (int lists = 0; lists < 2; lists++)
            for (int t = 0; t < 5; t++) {
                const auto t0 = std::chrono::steady_clock::now();
                CHECK(gsr_knn(ctx[0], knn_radius, knn_k, 0, 0, knn_stat, found.data(), lists ? idx.data() : nullptr, lists ? d2.data() : nullptr, values.data(), knn_n,
                              hist.data(), &knn_info));
                knn_ms[lists] = std::min(knn_ms[lists], std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
                float stage[2] = {0, 0};
                CHECK(gsr_debug_knn_times(ctx[0], stage));
                knn_index_ms[lists] = std::min(knn_index_ms[lists], (double)stage[0]); knn_walk_ms[lists] = std::min(knn_walk_ms[lists], (double)stage[1]);
            }
        double sum = 0;
        for (uint32_t i = 0; i < knn_n; i++) if (std::isfinite(values[i])) sum += values[i];
        knn_lo = knn_info.finite_values ? sum / (double)knn_info.finite_values : 0.0;
        for (uint32_t i = 0; i < knn_n; i++) knn_above += values[i] >= knn_lo;
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(gsr_select_knn(ctx[0], knn_radius, knn_k, 0, 0, knn_stat, knn_lo, HUGE_VAL, GSR_SELOP_REPLACE, &knn_selected, nullptr));
        knn_select_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    }
    // --normals: every splat's normal and surface variation, the stages timed apart, the pick checked against the variations
    gsr_normal_info nm_info{};
    double nm_ms = 1e30, nm_index_ms = 1e30, nm_walk_ms = 1e30, nm_select_ms = 0, nm_hi = 0;
    uint32_t nm_selected = 0, nm_n = 0;
    unsigned long long nm_within = 0;
    if (normals_radius > 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &nm_n));
        gsr_normal_options no{};
        no.source = normals_own ? GSR_NORMAL_OWN : GSR_NORMAL_KNN;
        no.k = normals_k; no.radius = normals_radius;
        std::vector<float> normals((size_t)nm_n * 3);
        std::vector<double> variation(nm_n);
        std::vector<uint32_t> found(nm_n);
        for (int t = 0; t < 5; t++) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_normals(ctx[0], &no, normals.data(), variation.data(), found.data(), nm_n, &nm_info));
            nm_ms = std::min(nm_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
            float stage[2] = {0, 0};
            CHECK(gsr_debug_normals_times(ctx[0], stage));
            nm_index_ms = std::min(nm_index_ms, (double)stage[0]); nm_walk_ms = std::min(nm_walk_ms, (double)stage[1]);
        }
        double sum = 0;
        for (uint32_t i = 0; i < nm_n; i++) if (!std::isnan(variation[i])) sum += variation[i];
        nm_hi = nm_info.valid ? sum / (double)nm_info.valid : 0.0;
        for (uint32_t i = 0; i < nm_n; i++) nm_within += variation[i] >= 0.0 && variation[i] <= nm_hi;
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(gsr_select_normal(ctx[0], &no, GSR_NORMAL_VARIATION, nullptr, 0.0, nm_hi, GSR_SELOP_REPLACE, &nm_selected, nullptr));
        nm_select_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
    }
    // --register: the scene registered to a moved copy of itself in a second context, the stages timed apart
    gsr_register_info reg_info{};
    std::vector<uint64_t> reg_step_pairs(reg_steps, 0);
    std::vector<double> reg_step_rms(reg_steps, 0.0);
    double reg_ms = 0, reg_M[12] = {0};
    float reg_stage[8] = {0};
    uint32_t reg_n = 0, reg_target_n = 0;
    gsr_register_surface_info rs_info{};
    std::vector<uint64_t> rs_step_pairs(rs_steps, 0), rs_step_surface_pairs(rs_steps, 0);
    std::vector<double> rs_step_rms(rs_steps, 0.0), rs_step_surface_rms(rs_steps, 0.0);
    double rs_ms = 0, rs_M[12] = {0};
    float rs_stage[8] = {0}, rs_normals[2] = {0};
    if (reg_radius > 0.0 || rs_radius > 0.0) {
        gsr_ctx* tgt = nullptr;
        gsr_options o{};
        o.device = 0; o.width = cfg->w; o.height = cfg->h;
        const int rc = gsr_create(&tgt, &o);
        if (rc) { std::fprintf(stderr, "gsr_create failed (%d): %s\n", rc, gsr_last_error(nullptr)); return 1; }
        ctx0 = tgt;
        CHECK(gsr_set_scene_rows(tgt, rows.data(), n));
        const double half = 0.005, al = std::sqrt(0.3 * 0.3 + 0.9 * 0.9 + 0.2 * 0.2), sh = std::sin(half);
        const double q[4] = {0.3 / al * sh, 0.9 / al * sh, 0.2 / al * sh, std::cos(half)}, tr[3] = {0.01, -0.005, 0.008};
        CHECK(gsr_scene_rotate(tgt, q));
        CHECK(gsr_scene_translate(tgt, tr));
        CHECK(gsr_scene_count(tgt, &reg_target_n));
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &reg_n));
        if (reg_radius > 0.0) {
            reg_info.step_pairs = reg_step_pairs.data(); reg_info.step_rms = reg_step_rms.data(); reg_info.step_rows = reg_steps;
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_register(ctx[0], tgt, nullptr, reg_radius, 0, 0, 0, reg_steps, 1.0 / 1099511627776.0, reg_M, &reg_info));
            reg_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
            CHECK(gsr_debug_match_times(ctx[0], reg_stage));
        }
        if (rs_radius > 0.0) {
            gsr_normal_options no{};
            no.source = rs_k ? GSR_NORMAL_KNN : GSR_NORMAL_OWN; no.k = rs_k; no.radius = rs_radius;
            rs_info.step_pairs = rs_step_pairs.data(); rs_info.step_surface_pairs = rs_step_surface_pairs.data();
            rs_info.step_rms = rs_step_rms.data(); rs_info.step_surface_rms = rs_step_surface_rms.data(); rs_info.step_rows = rs_steps;
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_register_surface(ctx[0], tgt, nullptr, rs_radius, 0, 0, 0, &no, rs_steps, 1.0 / 1099511627776.0, rs_M, &rs_info));
            rs_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
            CHECK(gsr_debug_match_times(ctx[0], rs_stage));
            ctx0 = tgt;
            CHECK(gsr_debug_normals_times(tgt, rs_normals));
            ctx0 = ctx[0];
        }
        gsr_destroy(tgt);
    }
    // --duplicate (last of all: it grows the scene): the selection duplicated on the device, twice
    double duplicate_ms = 0, duplicate_again_ms = 0, reserve_ms = 0;
    uint32_t dup_selected = 0, dup_first = 0, dup_count = 0, dup_capacity = 0, dup_n = 0;
    if (duplicate_fraction >= 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &dup_n));
        std::vector<uint32_t> words((dup_n + 31) / 32, 0u);
        const uint64_t limit = (uint64_t)(duplicate_fraction * 4294967296.0);
        for (uint32_t i = 0; i < dup_n; i++)
            if ((uint64_t)((i + 0x85ebca6bu) * 2654435761u) < limit) words[i >> 5] |= 1u << (i & 31);
        auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count() * 1e3; };
        CHECK(gsr_selection_set(ctx[0], words.data(), (uint32_t)words.size(), GSR_SELOP_REPLACE, &dup_selected));
        auto t = std::chrono::steady_clock::now();
        if (reserve) { CHECK(gsr_scene_reserve(ctx[0], dup_n + 2 * dup_selected)); reserve_ms = ms_since(t); }
        t = std::chrono::steady_clock::now();
        CHECK(gsr_scene_duplicate_selected(ctx[0], &dup_first, &dup_count));
        duplicate_ms = ms_since(t);
        t = std::chrono::steady_clock::now();
        CHECK(gsr_scene_duplicate_selected(ctx[0], nullptr, nullptr));
        duplicate_again_ms = ms_since(t);
        CHECK(gsr_scene_capacity(ctx[0], &dup_capacity));
        CHECK(gsr_scene_count(ctx[0], &dup_n));
    }
    // --merge (after everything else: it replaces the scene): the report three times, then the one blocking edit it announced
    gsr_cell_info mg_report{}, mg_info{};
    double mg_cells_ms = 1e30, mg_merge_ms = 0;
    uint32_t mg_before = 0, mg_after = 0, mg_selected = 0;
    if (merge_cell > 0.0) {
        ctx0 = ctx[0];
        CHECK(gsr_scene_count(ctx[0], &mg_before));
        for (int t = 0; t < 3; t++) {
            const auto t0 = std::chrono::steady_clock::now();
            CHECK(gsr_cells(ctx[0], merge_cell, 64, 0, 0, nullptr, 0, nullptr, &mg_report));
            mg_cells_ms = std::min(mg_cells_ms, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
        }
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(gsr_scene_merge_cells(ctx[0], merge_cell, 0, 0, &mg_after, &mg_info));
        mg_merge_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
        CHECK(gsr_read_selection(ctx[0], nullptr, 0, &mg_selected));
    }
    char name[128] = "";
    int32_t cus = 0, khz = 0;
    (void)gsr_device_info(ctx[0], name, (int32_t)sizeof name, &cus, &khz);
    std::printf("{\"caller\": \"C++ (tools/bench_cabi.cpp)\", \"config\": \"%s\", \"n\": %u, \"width\": %d, \"height\": %d, "
                "\"frames\": %d, \"warmup\": %d, \"frames_in_flight\": %d, \"frames_per_sec\": %.1f, \"ms_per_frame\": %.4f, "
                "\"rows_fnv1a\": \"%016llx\", \"depth_index_fnv1a\": \"%016llx\", \"rgba8_fnv1a\": \"%016llx\", \"device\": \"%s\", \"compute_units\": %d",
                cfg->name, n, cfg->w, cfg->h, frames, warmup, in_flight, frames / sec, sec / frames * 1e3,
                (unsigned long long)fnv1a(rows.data(), rows.size()), (unsigned long long)fnv1a(di.data(), di.size() * 4),
                (unsigned long long)fnv1a(px.data(), px.size()), name, cus);
    if (deliver && format == GSR_FORMAT_RGBA8)
        std::printf(", \"frames_per_sec_delivered\": %.1f, \"delivery_slots\": 3, \"delivered_rgba8_fnv1a\": \"%016llx\", "
                    "\"delivered_equals_read_pixels\": true, \"sink\": %d",
                    frames / delivered_sec, delivered_hash, (int)(sink & 1));
    else if (deliver)
        std::printf(", \"frames_per_sec_delivered\": %.1f, \"delivery_slots\": 3, \"delivery_format\": \"%s\", "
                    "\"delivered_payload_fnv1a\": \"%016llx\", \"sink\": %d",
                    frames / delivered_sec, deliver_format.c_str(), delivered_hash, (int)(sink & 1));
    if (deliver && depth_format != GSR_DEPTH_NONE)
        std::printf(", \"delivery_depth\": \"%s\", \"depth_step\": %d, \"depth_near\": %.9g, \"depth_width\": %d, \"depth_height\": %d, "
                    "\"depth_bytes\": %llu, \"delivered_depth_fnv1a\": \"%016llx\"",
                    deliver_depth.c_str(), dlay.step, (double)dlay.near, dlay.width, dlay.height, (unsigned long long)dlay.bytes, delivered_depth_hash);
    if (overlay_fraction >= 0.0) {
        std::printf(", \"overlay_fraction\": %g, \"overlay_selected\": %u, \"frames_per_sec_without_overlay\": %.1f, \"frames_per_sec_with_overlay\": %.1f, "
                    "\"overlay_legs\": 3, \"overlay_pass_us\": %.1f, \"overlay_rgba8_fnv1a\": \"%016llx\", \"overlay_cover_fnv1a\": \"%016llx\"",
                    overlay_fraction, overlay_selected, 3.0 * frames / overlay_sec[0], 3.0 * frames / overlay_sec[1], overlay_pass_us, overlay_hash[0], overlay_hash[1]);
        if (outline_width) std::printf(", \"outline_width\": %d", outline_width);
        if (depth) std::printf(", \"depth_pass_us\": %.1f", overlay_depth_pass_us);
    }
    if (contrib) {
        std::printf(", \"frames_per_sec_without_contrib\": %.1f, \"frames_per_sec_with_contrib\": %.1f, \"contrib_legs\": 3, \"contrib_pass_ms\": %.4f, "
                    "\"contrib_frames\": %u, \"contrib_weight_fnv1a\": \"%016llx\", \"contrib_peak_fnv1a\": \"%016llx\", \"contrib_pixels_fnv1a\": \"%016llx\"",
                    3.0 * frames / contrib_sec[0], 3.0 * frames / contrib_sec[1], contrib_pass_ms, contrib_frames, contrib_hash[0], contrib_hash[1], contrib_hash[2]);
        if (depth) std::printf(", \"depth_pass_ms\": %.4f", depth_pass_ms);
    }
    if (depth)
        std::printf(", \"frames_per_sec_plain\": %.1f, \"frames_per_sec_with_depth\": %.1f, \"depth_legs\": 3",
                    3.0 * frames / depth_sec[0], 3.0 * frames / depth_sec[1]);
    std::printf(", \"share_scene\": %s, \"scene_sharing\": {\"members\": %d, \"bytes\": %llu}, \"setup_ms\": %.2f",
                share_scene ? "true" : "false", share_members, (unsigned long long)share_bytes, setup_ms);
    if (hide_fraction >= 0.0) std::printf(", \"hide_fraction\": %g, \"hidden\": %u, \"hidden_set_ms\": %.3f", hide_fraction, hidden, hidden_set_ms);
    if (hide_edits)
        std::printf(", \"hide_edits\": {\"hide_selected_ms\": %.3f, \"erase_ms\": %.3f, \"erase_with_hidden_ms\": %.3f, \"hidden_after\": %u, \"kept\": %u}",
                    hide_selected_ms, erase_plain_ms, erase_hidden_ms, edits_hidden, edits_kept);
    if (scene_arrays) std::printf(", \"scene_from\": \"gsr_set_scene_arrays\"");
    if (scene_edit == "rotate") std::printf(", \"scene_edit\": \"rotate\", \"frames_per_sec_scene_edit\": %.1f", frames / edit_sec);
    if (edit_fraction >= 0.0)
        std::printf(", \"edit_selected_fraction\": %g, \"edit_selected\": %u, \"frames_per_sec_edit_selected\": %.1f, \"edit_ms\": %.4f", edit_fraction,
                    edit_selected, frames / edit_selected_sec, (edit_selected_sec - sec) / frames * 1e3);
    if (rotate_sh_fraction >= 0.0)
        std::printf(", \"rotate_sh\": {\"fraction\": %g, \"rows_all\": %u, \"all_ms\": %.4f, \"rows_selected\": %u, \"selected_ms\": %.4f, \"rotate_selected_sh_ms\": %.4f}",
                    rotate_sh_fraction, rotate_sh_rows_all, rotate_sh_all_ms, rotate_sh_rows, rotate_sh_selected_ms, rotate_selected_sh_ms);
    auto json_num = [](double v) -> std::string {   // (an empty box is (+inf, -inf): not JSON numbers)
        char buf[40];
        std::snprintf(buf, sizeof buf, "%.17g", v);
        return std::isfinite(v) ? std::string(buf) : std::string("null");
    };
    if (hist_attr >= 0)
        std::printf(", \"histogram\": {\"attr\": \"%s\", \"bins\": %u, \"count\": %u, \"nan\": %u, \"min\": %s, \"max\": %s, \"lo\": %.17g, \"hi\": %.17g, "
                    "\"below\": %u, \"above\": %u, \"nan_in_scope\": %u, \"largest_bin\": %llu, \"attr_stats_ms\": %.4f, \"attr_histogram_ms\": %.4f, "
                    "\"select_attr_ms\": %.4f, \"range\": [%u, %u], \"sum_counts\": %llu, \"selected\": %u, \"histogram_equals_selection\": %s}",
                    histogram_attr.c_str(), histogram_bins, hist_count, hist_nan, json_num(hist_min).c_str(), json_num(hist_max).c_str(), hist_lo, hist_hi, hist_outside[0], hist_outside[1], hist_outside[2],
                    hist_peak, hist_ms[0], hist_ms[1], hist_ms[2], hist_a, hist_b, hist_sum, hist_selected, hist_sum == hist_selected ? "true" : "false");
    if (plane_threshold >= 0.0)
        std::printf(", \"plane\": {\"threshold\": %.17g, \"hypotheses\": %u, \"in_scope\": %u, \"nonfinite\": %u, \"degenerate\": %u, \"found\": %u, \"best\": %u, "
                    "\"tests\": %llu, \"budget\": %llu, \"fit_plane_ms\": %.4f, \"candidates_ms\": %.4f, \"score_ms\": %.4f, \"tests_per_s\": %.4g, \"inliers\": %u, "
                    "\"plane\": [%.17g, %.17g, %.17g, %.17g], \"select_plane_ms\": %.4f, \"selected\": %u, \"fit_equals_selection\": %s}",
                    plane_threshold, plane_hypotheses, pl_info.in_scope, pl_info.nonfinite, pl_info.degenerate, pl_info.found, pl_info.best,
                    (unsigned long long)pl_info.tests, (unsigned long long)pl_info.budget, pl_ms, pl_cand_ms, pl_score_ms,
                    pl_score_ms > 0.0 ? (double)pl_info.tests / (pl_score_ms * 1e-3) : 0.0, pl_info.inliers, pl_info.plane[0], pl_info.plane[1], pl_info.plane[2],
                    pl_info.plane[3], pl_select_ms, pl_selected, pl_info.found && pl_selected == pl_info.inliers ? "true" : "false");
    if (nb_radius > 0.0)
        std::printf(", \"neighbours\": {\"radius\": %.17g, \"cap\": %u, \"n\": %u, \"in_scope\": %u, \"nonfinite\": %u, \"pair_bound\": %llu, \"budget\": %llu, "
                    "\"neighbours_ms\": %.4f, \"index_build_ms\": %.4f, \"count_ms\": %.4f, \"pair_tests_per_s\": %.4g, \"median_count\": %u, "
                    "\"fewer_than_3\": %llu, \"select_neighbours_ms\": %.4f, \"selected\": %u, \"histogram_equals_selection\": %s}",
                    nb_radius, nb_cap, nb_n, nb_info.in_scope, nb_info.nonfinite, (unsigned long long)nb_info.pair_bound, (unsigned long long)nb_info.budget, nb_ms,
                    nb_build_ms, nb_count_ms, nb_count_ms > 0 ? (double)nb_info.pair_bound / (nb_count_ms * 1e-3) : 0.0, nb_median, nb_few, nb_select_ms, nb_selected,
                    nb_few == nb_selected ? "true" : "false");
    if (cl_radius > 0.0)
        std::printf(", \"clusters\": {\"radius\": %.17g, \"min_pts\": %u, \"n\": %u, \"in_scope\": %u, \"nonfinite\": %u, \"pair_bound\": %llu, \"budget\": %llu, "
                    "\"clusters_ms\": %.4f, \"index_ms\": %.4f, \"core_ms\": %.4f, \"union_ms\": %.4f, \"border_ms\": %.4f, \"core\": %u, \"border\": %u, "
                    "\"noise\": %u, \"clusters\": %u, \"largest_label\": %u, \"largest_size\": %u, \"smaller_than_10\": %llu, \"select_clusters_ms\": %.4f, "
                    "\"selected\": %u, \"sizes_equal_selection\": %s}",
                    cl_radius, cl_min_pts, cl_n, cl_info.in_scope, cl_info.nonfinite, (unsigned long long)cl_info.pair_bound, (unsigned long long)cl_info.budget, cl_ms,
                    cl_stage_ms[0], cl_stage_ms[1], cl_stage_ms[2], cl_stage_ms[3], cl_info.core, cl_info.border, cl_info.noise, cl_info.clusters, cl_info.largest_label,
                    cl_info.largest_size, cl_small, cl_select_ms, cl_selected, cl_small == cl_selected ? "true" : "false");
    if (reg_radius > 0.0) {
        std::printf(", \"register\": {\"radius\": %.17g, \"max_iterations\": %u, \"n\": %u, \"target_n\": %u, \"status\": \"%s\", \"iterations\": %u, \"pairs\": %llu, "
                    "\"rms\": %s, \"delta\": %s, \"register_ms\": %.4f, \"index_build_ms\": %.4f, \"bound_ms\": %.4f, \"walk_ms\": %.4f, \"tree_ms\": %.4f, "
                    "\"steps_bound_ms\": %.4f, \"steps_walk_ms\": %.4f, \"steps_tree_ms\": %.4f, \"transform\": [",
                    reg_radius, reg_steps, reg_n, reg_target_n,
                    reg_info.status == GSR_REGISTER_CONVERGED ? "converged" : reg_info.status == GSR_REGISTER_TOO_FEW ? "too_few" : "max_iterations", reg_info.iterations,
                    (unsigned long long)reg_info.pairs, json_num(reg_info.rms).c_str(), json_num(reg_info.delta).c_str(), reg_ms, reg_stage[0], reg_stage[1], reg_stage[2],
                    reg_stage[3], reg_stage[4], reg_stage[5], reg_stage[6]);
        for (int k = 0; k < 12; k++) std::printf("%s%.17g", k ? ", " : "", reg_M[k]);
        std::printf("], \"step_pairs\": [");
        for (uint32_t k = 0; k < reg_info.iterations; k++) std::printf("%s%llu", k ? ", " : "", (unsigned long long)reg_step_pairs[k]);
        std::printf("], \"step_rms\": [");
        for (uint32_t k = 0; k < reg_info.iterations; k++) std::printf("%s%s", k ? ", " : "", json_num(reg_step_rms[k]).c_str());
        std::printf("]}");
    }
    if (rs_radius > 0.0) {
        std::printf(", \"register_surface\": {\"radius\": %.17g, \"max_iterations\": %u, \"normals\": \"%s\", \"k\": %u, \"n\": %u, \"target_n\": %u, \"status\": \"%s\", "
                    "\"iterations\": %u, \"pairs\": %llu, \"surface_pairs\": %llu, \"valid\": %u, \"rms\": %s, \"surface_rms\": %s, \"delta\": %s, "
                    "\"register_surface_ms\": %.4f, \"normals_index_ms\": %.4f, \"normals_walk_ms\": %.4f, \"index_build_ms\": %.4f, \"bound_ms\": %.4f, \"walk_ms\": %.4f, "
                    "\"rows_tree_ms\": %.4f, \"steps_bound_ms\": %.4f, \"steps_walk_ms\": %.4f, \"steps_rows_tree_ms\": %.4f, \"transform\": [",
                    rs_radius, rs_steps, rs_k ? "knn" : "own", rs_k, reg_n, reg_target_n,
                    rs_info.status == GSR_REGISTER_CONVERGED ? "converged" : rs_info.status == GSR_REGISTER_TOO_FEW ? "too_few"
                        : rs_info.status == GSR_REGISTER_DEGENERATE ? "degenerate" : "max_iterations",
                    rs_info.iterations, (unsigned long long)rs_info.pairs, (unsigned long long)rs_info.surface_pairs, rs_info.valid, json_num(rs_info.rms).c_str(),
                    json_num(rs_info.surface_rms).c_str(), json_num(rs_info.delta).c_str(), rs_ms, rs_normals[0], rs_normals[1], rs_stage[0], rs_stage[1], rs_stage[2],
                    rs_stage[3], rs_stage[4], rs_stage[5], rs_stage[6]);
        for (int k = 0; k < 12; k++) std::printf("%s%.17g", k ? ", " : "", rs_M[k]);
        std::printf("], \"step_pairs\": [");
        for (uint32_t k = 0; k < rs_info.iterations; k++) std::printf("%s%llu", k ? ", " : "", (unsigned long long)rs_step_pairs[k]);
        std::printf("], \"step_surface_pairs\": [");
        for (uint32_t k = 0; k < rs_info.iterations; k++) std::printf("%s%llu", k ? ", " : "", (unsigned long long)rs_step_surface_pairs[k]);
        std::printf("], \"step_rms\": [");
        for (uint32_t k = 0; k < rs_info.iterations; k++) std::printf("%s%s", k ? ", " : "", json_num(rs_step_rms[k]).c_str());
        std::printf("], \"step_surface_rms\": [");
        for (uint32_t k = 0; k < rs_info.iterations; k++) std::printf("%s%s", k ? ", " : "", json_num(rs_step_surface_rms[k]).c_str());
        std::printf("]}");
    }
    if (normals_radius > 0.0)
        std::printf(", \"normals\": {\"source\": \"%s\", \"radius\": %.17g, \"k\": %u, \"n\": %u, \"in_scope\": %u, \"nonfinite\": %u, \"pair_bound\": %llu, \"budget\": %llu, "
                    "\"normals_ms\": %.4f, \"index_build_ms\": %.4f, \"walk_ms\": %.4f, \"valid\": %u, \"variation_min\": %s, \"variation_max\": %s, "
                    "\"variation_hi\": %.17g, \"within\": %llu, \"select_normal_ms\": %.4f, \"selected\": %u, \"variation_equals_selection\": %s}",
                    normals_own ? "own" : "knn", normals_radius, normals_k, nm_n, nm_info.in_scope, nm_info.nonfinite, (unsigned long long)nm_info.pair_bound,
                    (unsigned long long)nm_info.budget, nm_ms, nm_index_ms, nm_walk_ms, nm_info.valid, json_num(nm_info.variation_min).c_str(),
                    json_num(nm_info.variation_max).c_str(), nm_hi, nm_within, nm_select_ms, nm_selected, nm_within == nm_selected ? "true" : "false");
    if (knn_radius > 0.0)
        std::printf(", \"knn\": {\"radius\": %.17g, \"k\": %u, \"stat\": \"%s\", \"n\": %u, \"in_scope\": %u, \"nonfinite\": %u, \"pair_bound\": %llu, \"budget\": %llu, "
                    "\"knn_ms\": %.4f, \"index_build_ms\": %.4f, \"walk_ms\": %.4f, \"pair_tests_per_s\": %.4g, \"knn_lists_ms\": %.4f, \"lists_index_build_ms\": %.4f, "
                    "\"lists_walk_ms\": %.4f, \"complete\": %u, \"finite_values\": %u, \"value_min\": %s, \"value_max\": %s, \"select_lo\": %.17g, "
                    "\"at_or_above\": %llu, \"select_knn_ms\": %.4f, \"selected\": %u, \"values_equal_selection\": %s}",
                    knn_radius, knn_k, knn_stat == GSR_KNN_KTH ? "kth" : "mean", knn_n, knn_info.in_scope, knn_info.nonfinite, (unsigned long long)knn_info.pair_bound,
                    (unsigned long long)knn_info.budget, knn_ms[0], knn_index_ms[0], knn_walk_ms[0], knn_walk_ms[0] > 0 ? (double)knn_info.pair_bound / (knn_walk_ms[0] * 1e-3) : 0.0,
                    knn_ms[1], knn_index_ms[1], knn_walk_ms[1], knn_info.complete, knn_info.finite_values, json_num(knn_info.value_min).c_str(),
                    json_num(knn_info.value_max).c_str(), knn_lo, knn_above, knn_select_ms, knn_selected, knn_above == knn_selected ? "true" : "false");
    if (duplicate_fraction >= 0.0)
        std::printf(", \"duplicate_fraction\": %g, \"duplicate_first\": %u, \"duplicate_count\": %u, \"duplicate_reserved\": %s, \"reserve_ms\": %.4f, "
                    "\"duplicate_ms\": %.4f, \"duplicate_again_ms\": %.4f, \"count_after\": %u, \"capacity_after\": %u",
                    duplicate_fraction, dup_first, dup_count, reserve ? "true" : "false", reserve_ms, duplicate_ms, duplicate_again_ms, dup_n, dup_capacity);
    if (merge_cell > 0.0)
        std::printf(", \"merge\": {\"cell\": %.17g, \"rows_before\": %u, \"rows_after\": %u, \"rows_announced\": %u, \"in_scope\": %u, \"candidates\": %u, "
                    "\"cells\": %u, \"merged_cells\": %u, \"merged_members\": %u, \"largest\": %u, \"members_per_cell\": %.3f, \"pair_bound\": %llu, \"budget\": %llu, "
                    "\"cells_ms\": %.4f, \"merge_blocking_ms\": %.4f, \"selected_after\": %u, \"report_equals_edit\": %s}",
                    merge_cell, mg_before, mg_after, mg_report.rows_after, mg_info.in_scope, mg_info.candidates, mg_info.cells, mg_info.merged_cells, mg_info.merged_members,
                    mg_info.largest, mg_info.cells ? (double)mg_info.candidates / mg_info.cells : 0.0, (unsigned long long)mg_info.pair_bound,
                    (unsigned long long)mg_info.budget, mg_cells_ms, mg_merge_ms, mg_selected,
                    mg_after == mg_report.rows_after && mg_selected == mg_info.merged_cells ? "true" : "false");
    if (pick)
        std::printf(", \"pick\": {\"x\": %d, \"y\": %d, \"index\": %u, \"depth\": %s, \"mean\": %.9g, \"alpha\": %.9g}",
                    pick_xy[0], pick_xy[1], picked.index, picked.index == 0xffffffffu ? "null" : std::to_string(picked.depth).c_str(), (double)picked.mean, (double)picked.alpha);
    std::printf("}\n");
    for (gsr_ctx* c : ctx) gsr_destroy(c);
    return 0;
}
