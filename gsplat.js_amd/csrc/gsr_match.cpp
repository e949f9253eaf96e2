// Matching and registration: for every splat in scope of this context's scene, moved by a trial transform, the nearest splat in
// scope of ANOTHER context's scene within a radius -- the match itself, the sums a rigid solve needs, the splats of a distance range
// as a picker -- and the rigid registration that iterates match, reduce and solve on the host (include/gsplat_hip.h, "matching and
// registration"; kernels: k_match.hip over k_neighbours.hip's index).  gsr_match, gsr_select_match and gsr_register are blocking
// and stateless: they wait for every member's stream of both contexts' shared scenes first, index the target's scene as it is now,
// read both scenes and write neither; gsr_select_match changes this context's selection the way every picker does.  The scratch
// is this context's: its neighbour scratch (gsr_neighbours.cpp) sized for the TARGET's count, 12 bytes per source splat for idx and
// d2, and the tree's partial rows once sums are asked for; the first call allocates it, it only grows, the context's end frees it.
// A context that never calls these allocates and launches nothing.  gsr_rigid_solve, gsr_rigid_compose and gsr_rigid_decompose
// are pure functions of their arguments and need no device.
//
// The work budget is the neighbour budget: the index is built, k_match_bound sums what the one 27-cell walk of the queries tests
// at most, and a step above its budget is refused before the walk is launched.  The target does not change between the steps of
// a gsr_register, so its index is built once per call; the bound depends on the trial transform and is taken at every step.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>
#include <limits>

using namespace gsr;

namespace {

constexpr uint32_t MATCH_INFO_WORDS = 12;
static_assert(sizeof(MatchInfo) <= MATCH_INFO_WORDS * 4, "MatchInfo fits its words");
static_assert(MATCH_NONE == GSR_MATCH_NONE, "the header's word");
static_assert(sizeof(gsr_match_info) == 48 && sizeof(gsr_match_sums) == 8 + MATCH_ROW * 8 && sizeof(gsr_register_info) == 56, "the header's layouts");
static_assert(sizeof(gsr_surface_sums) == 16 + MATCH_SURFACE_ROW * 8 && sizeof(gsr_register_surface_info) == 88, "the header's layouts");
constexpr double INF = std::numeric_limits<double>::infinity();
const double IDENTITY[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};

// the refusals the three calls share, in the header's order.  Nothing is touched by a refused call.
int match_check(gsr_ctx* c, gsr_ctx* target, const char* who, const double* M, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget)
{
    if (!target) return fail(c, GSR_ERR_ARG, "%s: target is NULL", who);
    if (c->device != target->device) return fail(c, GSR_ERR_ARG, "%s: the contexts are on different devices (%d and %d)", who, c->device, target->device);
    if (int r = nb_check(c, who, radius, 1u, scope, budget)) return r;
    if (int r = scope_check(c, who, target_scope)) return r;
    if (M)
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(M[k])) return fail(c, GSR_ERR_ARG, "%s: entry %d of the transform is %g: it must be finite", who, k, M[k]);
    return GSR_OK;
}

// which tree a step ends with: none, the sixteen sums of the rigid solve, the 29 of the point-to-plane solve
enum MatchTree { TREE_NONE, TREE_POINT, TREE_SURFACE };

// the context's scratch for n source splats, with the rows of the tree asked for: allocated by the first call, only ever grown
int match_ensure(gsr_ctx* c, uint32_t n, MatchTree tree)
{
    gsr_ctx::Match& mt = c->mt;
    if (!mt.words) { if (int r = mt.words.alloc(c, MATCH_INFO_WORDS)) return r; }
    if (mt.rows < n || !mt.idx) {
        mt.rows = 0;
        int r;
        if ((r = mt.idx.alloc(c, n)) || (r = mt.d2.alloc(c, n))) return r;
        mt.rows = n;
    }
    const uint64_t rows = tree != TREE_NONE && n ? match_tree_rows(n) : 0u;
    if (rows && tree == TREE_POINT && (mt.tree_rows < rows || !mt.tree)) {
        mt.tree_rows = 0;
        if (int r = mt.tree.alloc(c, (size_t)rows * MATCH_ROW)) return r;
        mt.tree_rows = rows;
    }
    if (rows && tree == TREE_SURFACE && (mt.surface_rows < rows || !mt.surface_tree)) {
        mt.surface_rows = 0;
        if (int r = mt.surface_tree.alloc(c, (size_t)rows * MATCH_SURFACE_ROW)) return r;
        mt.surface_rows = rows;
    }
    for (hipEvent_t& e : mt.ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
    return GSR_OK;
}

gsr_match_info match_zero_info(uint64_t budget)
{
    gsr_match_info z{};
    z.budget = budget;
    z.d2_min = INF;
    z.d2_max = -INF;
    return z;
}

struct MatchCall {
    NbIndex ix;
    uint32_t indexed;                       // the target index's entries
    MatchSource src;                        // (xf: set per step)
    const float *qx, *qy, *qz;              // the target's positions
    uint32_t tn;
    uint64_t budget;
    double radius;
};

// Everything that does not depend on the trial transform: both scenes settled, the scratch, the index over the target.  The
// source scene holds n >= 1 splats; the device is current afterwards and no member's stream of either scene holds work.
int match_index(gsr_ctx* c, gsr_ctx* target, const char* who, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, MatchTree tree, MatchCall* call,
                gsr_match_info* info)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    if (target->scene != c->scene)
        for (gsr_ctx* m : target->scene->members) HIP_TRY(c, hipStreamSynchronize(m->stream));
    const SharedScene& sc = *c->scene;
    const SharedScene& ts = *target->scene;
    const uint32_t n = sc.n, tn = ts.n;
    if (int r = match_ensure(c, n, tree)) return r;
    MatchCall k{};
    uint32_t* hist = nullptr;
    if (int r = nb_prepare_rows(c, who, tn ? tn : 1u, 0u, 1.0 / (radius * (1.0 + 1.0 / 1024.0)), radius * radius, &k.ix, &hist)) return r;
    gsr_ctx::Match& mt = c->mt;
    for (float& v : mt.ms) v = 0.0f;
    HIP_TRY(c, hipEventRecord(mt.ev[0], c->stream));
    // (an empty target: the zeroed table is the index of nothing, every bucket's range empty)
    if (tn) launch_nb_build(k.ix, ts.arr.px, ts.arr.py, ts.arr.pz, scene_scope(ts, target_scope), tn, c->cu_count, nullptr, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(mt.ev[1], c->stream);
    NbInfo got{};
    hipError_t e2 = hipMemcpyAsync(&got, k.ix.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (got.indexed > tn || got.indexed != got.in_scope - got.nonfinite)
        return fail(c, GSR_ERR_HIP, "%s: the index holds %u entries for %u target splats in scope, %u of them non-finite", who, got.indexed, got.in_scope, got.nonfinite);
    k.indexed = got.indexed;
    k.src = MatchSource{sc.arr.px, sc.arr.py, sc.arr.pz, scene_scope(sc, scope), n, MatchXf{}};
    k.qx = ts.arr.px; k.qy = ts.arr.py; k.qz = ts.arr.pz;
    k.tn = tn;
    k.budget = budget;
    k.radius = radius;
    info->target_indexed = got.indexed;
    *call = k;
    return GSR_OK;
}

// One step under the transform M: the bound against the budget, the walk, the tree the caller chose (sums non-null: the sixteen
// sums; surface non-null: the 29 along `normals`, the target's stored rows, final on the device) and *info, final on the device and
// waited for.  GSR_ERR_ARG (with *info's first fields filled) for a bound above the budget: no walk has been launched.
int match_step(gsr_ctx* c, const char* who, MatchCall* call, const double* M, gsr_match_sums* sums, gsr_match_info* info, const float* normals = nullptr,
               gsr_surface_sums* surface = nullptr)
{
    gsr_ctx::Match& mt = c->mt;
    std::memcpy(call->src.xf.m, M ? M : IDENTITY, sizeof call->src.xf.m);
    MatchInfo* dev = reinterpret_cast<MatchInfo*>(mt.words.p);
    HIP_TRY(c, hipMemsetAsync(mt.words, 0, MATCH_INFO_WORDS * 4, c->stream));
    HIP_TRY(c, hipEventRecord(mt.ev[2], c->stream));
    launch_match_bound(call->ix, call->src, dev, c->cu_count, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(mt.ev[3], c->stream);
    MatchInfo got{};
    hipError_t e2 = hipMemcpyAsync(&got, dev, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    info->in_scope = got.in_scope; info->nonfinite = got.nonfinite; info->pair_bound = got.pair_bound; info->budget = call->budget;
    info->matched = 0u; info->d2_min = INF; info->d2_max = -INF;
    if (got.nonfinite > got.in_scope || got.in_scope > call->src.n)
        return fail(c, GSR_ERR_HIP, "%s: %u splats in scope of %u, %u of them non-finite", who, got.in_scope, call->src.n, got.nonfinite);
    if (got.pair_bound > call->budget)
        return fail(c, GSR_ERR_ARG, "%s: the walk would make up to %llu pair tests, above the budget of %llu (radius %g puts too many target splats into one cell)",
                    who, (unsigned long long)got.pair_bound, (unsigned long long)call->budget, call->radius);
    launch_match(call->ix, call->indexed, call->src, mt.idx, mt.d2, dev, c->cu_count, c->stream);
    e0 = hipGetLastError();
    e1 = hipEventRecord(mt.ev[4], c->stream);
    double row[MATCH_ROW] = {}, srow[MATCH_SURFACE_ROW] = {};
    hipError_t e4 = hipSuccess, e5 = hipSuccess;
    if (surface) {
        launch_match_surface_tree(call->src, call->qx, call->qy, call->qz, normals, call->tn, mt.idx, mt.d2, mt.surface_tree, dev, c->stream);
        e4 = hipGetLastError();
        e5 = hipMemcpyAsync(srow, mt.surface_tree + (match_tree_rows(call->src.n) - 1u) * MATCH_SURFACE_ROW, sizeof srow, hipMemcpyDeviceToHost, c->stream);
    } else if (sums) {
        launch_match_tree(call->src, call->qx, call->qy, call->qz, call->tn, mt.idx, mt.d2, mt.tree, c->stream);
        e4 = hipGetLastError();
        e5 = hipMemcpyAsync(row, mt.tree + (match_tree_rows(call->src.n) - 1u) * MATCH_ROW, sizeof row, hipMemcpyDeviceToHost, c->stream);
    }
    hipError_t e6 = hipEventRecord(mt.ev[5], c->stream);
    e2 = hipMemcpyAsync(&got, dev, sizeof got, hipMemcpyDeviceToHost, c->stream);
    e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e4, e5, e6, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (got.matched > got.in_scope - got.nonfinite)
        return fail(c, GSR_ERR_HIP, "%s: %u matches for %u queries", who, got.matched, got.in_scope - got.nonfinite);
    if (got.surface > got.matched || (!surface && got.surface))
        return fail(c, GSR_ERR_HIP, "%s: %u rows along a normal for %u matches", who, got.surface, got.matched);
    info->matched = got.matched;
    if (got.matched) {
        const uint64_t lo = ~(uint64_t)got.nd2min, hi = (uint64_t)got.d2max;
        std::memcpy(&info->d2_min, &lo, 8);
        std::memcpy(&info->d2_max, &hi, 8);
    }
    if (sums) {
        sums->pairs = got.matched;
        std::memcpy(sums->sum, row, sizeof row);
    }
    if (surface) {
        surface->pairs = got.matched;
        surface->surface_pairs = got.surface;
        std::memcpy(surface->sum, srow, sizeof srow);
    }
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool ok = hipEventElapsedTime(&ms[0], mt.ev[0], mt.ev[1]) == hipSuccess;
    for (int k = 1; k < 4; k++) ok = hipEventElapsedTime(&ms[k], mt.ev[k + 1], mt.ev[k + 2]) == hipSuccess && ok;
    if (ok) {
        std::memcpy(mt.ms, ms, sizeof ms);
        for (int k = 1; k < 4; k++) mt.ms[3 + k] += ms[k];
        mt.ms[7] += 1.0f;
    } else (void)hipGetLastError();
    return GSR_OK;
}

double step_rms(const gsr_match_sums& s) { return s.pairs ? std::sqrt(s.sum[15] * (1.0 / (double)s.pairs)) : INF; }

// What the two point-to-plane calls do between their refusals and their steps: the target's normals as gsr_normals(target,
// options) stores them, by normal_run into TARGET's scratch.  Both scenes are settled first; normal_run waits for the target's
// stream, so the rows kernel on c's stream reads final rows.  A message of the target's side becomes c's.  ts.n >= 1.
int surface_normals(gsr_ctx* c, gsr_ctx* target, const char* who, const gsr_normal_options* o, const float** normals, uint32_t* valid)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    if (target->scene != c->scene)
        if (int r = settle_members(target)) return fail(c, r, "%s: the target: %s", who, gsr_last_error(target));
    NormalArrays a{};
    gsr_normal_info ni{};
    ni.budget = o->budget ? o->budget : GSR_NEIGHBOUR_DEFAULT_BUDGET;
    if (int r = normal_run(target, who, o, ni.budget, &a, &ni)) return target == c ? r : fail(c, r, "%s", gsr_last_error(target));
    HIP_TRY(c, hipStreamSynchronize(target->stream));   // (normal_run has waited: the order stated where the rows are read)
    *normals = a.normals;
    *valid = ni.valid;
    return GSR_OK;
}

// the refusals of the point-to-plane calls behind match_check's: gsr_normals' on the target, and the one scope
int surface_check(gsr_ctx* c, gsr_ctx* target, const char* who, uint32_t target_scope, const gsr_normal_options* o)
{
    if (!o) return fail(c, GSR_ERR_ARG, "%s: options is NULL", who);
    if (int r = normal_check(target, who, o)) return target == c ? r : fail(c, r, "%s", gsr_last_error(target));
    if (o->scope != target_scope) return fail(c, GSR_ERR_ARG, "%s: options->scope (%u) is not target_scope (%u)", who, o->scope, target_scope);
    if (o->source == GSR_NORMAL_OWN && target->scene->n)
        if (int r = require_rows(target)) return target == c ? r : fail(c, r, "%s: the target: %s", who, gsr_last_error(target));
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_match(gsr_ctx* c, gsr_ctx* target, const double* M, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, uint32_t* idx, double* d2,
              uint32_t n, gsr_match_sums* sums, gsr_match_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = match_check(c, target, "gsr_match", M, radius, scope, target_scope, budget)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    const SharedScene& sc = *c->scene;
    if ((idx || d2) && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_match: n (%u) is not the scene's count (%u)", n, sc.n);
    gsr_match_info got = match_zero_info(budget);
    if (sums) *sums = gsr_match_sums{};
    if (!sc.n) {
        if (info) *info = got;
        return GSR_OK;
    }
    MatchCall call;
    int r = match_index(c, target, "gsr_match", radius, scope, target_scope, budget, sums ? TREE_POINT : TREE_NONE, &call, &got);
    if (!r) r = match_step(c, "gsr_match", &call, M, sums, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    const gsr_ctx::Match& mt = c->mt;
    hipError_t e0 = idx ? hipMemcpyAsync(idx, mt.idx, (size_t)sc.n * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e1 = d2 ? hipMemcpyAsync(d2, mt.d2, (size_t)sc.n * 8, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_match failed: %s", hipGetErrorString(e));
    return GSR_OK;
}

int gsr_select_match(gsr_ctx* c, gsr_ctx* target, const double* M, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, double lo, double hi,
                     int32_t op, uint32_t* selected, gsr_match_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = match_check(c, target, "gsr_select_match", M, radius, scope, target_scope, budget)) return r;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_match: unknown op %d", op);
    if (std::isnan(lo) || std::isnan(hi) || lo > hi) return fail(c, GSR_ERR_ARG, "gsr_select_match: [%g, %g) must satisfy lo <= hi, neither a NaN", lo, hi);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    gsr_match_info got = match_zero_info(budget);
    if (!sc.n) {
        if (selected) *selected = 0;
        if (info) *info = got;
        return GSR_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    if (int r = select_ensure(c)) return r;   // (in front of the scope: a selection never allocated becomes the zeroed mask, the same set)
    MatchCall call;
    int r = match_index(c, target, "gsr_select_match", radius, scope, target_scope, budget, TREE_NONE, &call, &got);
    if (!r) r = match_step(c, "gsr_select_match", &call, M, nullptr, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    launch_match_select(c->mt.d2, call.src.sc, sc.n, lo, hi, hi == INF, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    return select_fold_and_count(c, op, selected);
}

int gsr_register(gsr_ctx* c, gsr_ctx* target, const double* M0, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget, uint32_t max_iterations,
                 double tolerance, double* M_out, gsr_register_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = match_check(c, target, "gsr_register", M0, radius, scope, target_scope, budget)) return r;
    if (std::isnan(tolerance) || tolerance < 0.0) return fail(c, GSR_ERR_ARG, "gsr_register: tolerance (%g) must be >= 0 and no NaN", tolerance);
    if (max_iterations < 1u || max_iterations > GSR_REGISTER_MAX_ITERATIONS_LIMIT)
        return fail(c, GSR_ERR_ARG, "gsr_register: max_iterations (%u) must be in 1 .. %u", max_iterations, GSR_REGISTER_MAX_ITERATIONS_LIMIT);
    uint64_t* step_pairs = info ? info->step_pairs : nullptr;
    double* step_rms_out = info ? info->step_rms : nullptr;
    if ((step_pairs || step_rms_out) && info->step_rows < max_iterations)
        return fail(c, GSR_ERR_ARG, "gsr_register: step_rows (%u) is below max_iterations (%u)", info->step_rows, max_iterations);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    double M[12];
    std::memcpy(M, M0 ? M0 : IDENTITY, sizeof M);
    gsr_register_info out{};
    if (info) out = *info;
    out.status = GSR_REGISTER_MAX_ITERATIONS; out.iterations = 0u; out.pairs = 0u; out.rms = INF; out.delta = INF; out.reserved = 0u;
    const SharedScene& sc = *c->scene;
    MatchCall call;
    gsr_match_info mi = match_zero_info(budget);
    if (sc.n)
        if (int r = match_index(c, target, "gsr_register", radius, scope, target_scope, budget, TREE_POINT, &call, &mi)) return r;
    for (uint32_t t = 0; t < max_iterations; t++) {
        gsr_match_sums sums{};
        if (sc.n)   // (an empty scene: a step of zeros)
            if (int r = match_step(c, "gsr_register", &call, M, &sums, &mi)) return r;
        out.iterations = t + 1u; out.pairs = sums.pairs; out.rms = step_rms(sums);
        if (step_pairs) step_pairs[t] = sums.pairs;
        if (step_rms_out) step_rms_out[t] = out.rms;
        if (sums.pairs < 3u) { out.status = GSR_REGISTER_TOO_FEW; break; }
        double D[12];
        if (gsr_rigid_solve(&sums, D, nullptr)) return fail(c, GSR_ERR_HIP, "gsr_register: step %u left sums that are not finite", t);
        double delta = 0.0;
        for (int k = 0; k < 12; k++) delta = std::fmax(delta, std::fabs(D[k] - IDENTITY[k]));
        out.delta = delta;
        gsr_rigid_compose(D, M, M);
        if (delta <= tolerance) { out.status = GSR_REGISTER_CONVERGED; break; }
    }
    if (M_out) std::memcpy(M_out, M, sizeof M);
    if (info) *info = out;
    return GSR_OK;
}

int gsr_match_surface(gsr_ctx* c, gsr_ctx* target, const double* M, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget,
                      const gsr_normal_options* o, gsr_surface_sums* sums, gsr_match_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = match_check(c, target, "gsr_match_surface", M, radius, scope, target_scope, budget)) return r;
    if (int r = surface_check(c, target, "gsr_match_surface", target_scope, o)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    const SharedScene& sc = *c->scene;
    gsr_match_info got = match_zero_info(budget);
    if (sums) *sums = gsr_surface_sums{};
    if (!sc.n) {
        if (info) *info = got;
        return GSR_OK;
    }
    const float* normals = nullptr;
    uint32_t valid = 0u;
    if (target->scene->n)   // (an empty target matches nothing: no row reads a normal)
        if (int r = surface_normals(c, target, "gsr_match_surface", o, &normals, &valid)) return r;
    MatchCall call;
    gsr_surface_sums s{};
    int r = match_index(c, target, "gsr_match_surface", radius, scope, target_scope, budget, TREE_SURFACE, &call, &got);
    if (!r) r = match_step(c, "gsr_match_surface", &call, M, nullptr, &got, normals, &s);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    if (sums) *sums = s;
    return GSR_OK;
}

int gsr_register_surface(gsr_ctx* c, gsr_ctx* target, const double* M0, double radius, uint32_t scope, uint32_t target_scope, uint64_t budget,
                         const gsr_normal_options* o, uint32_t max_iterations, double tolerance, double* M_out, gsr_register_surface_info* info)
{
    static const char* who = "gsr_register_surface";
    if (!c) return GSR_ERR_ARG;
    if (int r = match_check(c, target, who, M0, radius, scope, target_scope, budget)) return r;
    if (std::isnan(tolerance) || tolerance < 0.0) return fail(c, GSR_ERR_ARG, "%s: tolerance (%g) must be >= 0 and no NaN", who, tolerance);
    if (max_iterations < 1u || max_iterations > GSR_REGISTER_MAX_ITERATIONS_LIMIT)
        return fail(c, GSR_ERR_ARG, "%s: max_iterations (%u) must be in 1 .. %u", who, max_iterations, GSR_REGISTER_MAX_ITERATIONS_LIMIT);
    if (info && (info->step_pairs || info->step_surface_pairs || info->step_rms || info->step_surface_rms) && info->step_rows < max_iterations)
        return fail(c, GSR_ERR_ARG, "%s: step_rows (%u) is below max_iterations (%u)", who, info->step_rows, max_iterations);
    if (int r = surface_check(c, target, who, target_scope, o)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    double M[12];
    std::memcpy(M, M0 ? M0 : IDENTITY, sizeof M);
    gsr_register_surface_info out{};
    if (info) out = *info;
    out.status = GSR_REGISTER_MAX_ITERATIONS; out.iterations = 0u; out.pairs = 0u; out.surface_pairs = 0u; out.rms = INF; out.surface_rms = INF; out.delta = INF;
    out.valid = 0u;
    const SharedScene& sc = *c->scene;
    MatchCall call;
    gsr_match_info mi = match_zero_info(budget);
    const float* normals = nullptr;
    if (sc.n) {
        if (target->scene->n)
            if (int r = surface_normals(c, target, who, o, &normals, &out.valid)) return r;
        if (int r = match_index(c, target, who, radius, scope, target_scope, budget, TREE_SURFACE, &call, &mi)) return r;
    }
    for (uint32_t t = 0; t < max_iterations; t++) {
        gsr_surface_sums sums{};
        if (sc.n)   // (an empty scene: a step of zeros)
            if (int r = match_step(c, who, &call, M, nullptr, &mi, normals, &sums)) return r;
        out.iterations = t + 1u; out.pairs = sums.pairs; out.surface_pairs = sums.surface_pairs;
        out.rms = sums.pairs ? std::sqrt(sums.sum[28] * (1.0 / (double)sums.pairs)) : INF;
        out.surface_rms = sums.surface_pairs ? std::sqrt(sums.sum[27] * (1.0 / (double)sums.surface_pairs)) : INF;
        if (out.step_pairs) out.step_pairs[t] = sums.pairs;
        if (out.step_surface_pairs) out.step_surface_pairs[t] = sums.surface_pairs;
        if (out.step_rms) out.step_rms[t] = out.rms;
        if (out.step_surface_rms) out.step_surface_rms[t] = out.surface_rms;
        if (sums.surface_pairs < 6u) { out.status = GSR_REGISTER_TOO_FEW; break; }
        double D[12];
        int32_t degenerate = 0;
        if (gsr_surface_solve(&sums, D, nullptr, &degenerate)) return fail(c, GSR_ERR_HIP, "%s: step %u left sums that are not finite", who, t);
        if (degenerate) { out.status = GSR_REGISTER_DEGENERATE; break; }
        double delta = 0.0;
        for (int k = 0; k < 12; k++) delta = std::fmax(delta, std::fabs(D[k] - IDENTITY[k]));
        out.delta = delta;
        gsr_rigid_compose(D, M, M);
        if (delta <= tolerance) { out.status = GSR_REGISTER_CONVERGED; break; }
    }
    if (M_out) std::memcpy(M_out, M, sizeof M);
    if (info) *info = out;
    return GSR_OK;
}

// The 6 x 6 normal equations of the point-to-plane residuals by Cholesky, and the Cayley step, in the header's written order.
// f64; no context, no device.
int gsr_surface_solve(const gsr_surface_sums* sums, double* D, double* rms, int32_t* degenerate)
{
    if (!sums || !D || !degenerate) return fail(nullptr, GSR_ERR_ARG, "gsr_surface_solve: a NULL pointer");
    if (sums->surface_pairs < 6u)
        return fail(nullptr, GSR_ERR_ARG, "gsr_surface_solve: %llu pairs with a normal: at least 6 are needed", (unsigned long long)sums->surface_pairs);
    for (uint32_t k = 0; k < MATCH_SURFACE_ROW; k++)
        if (!std::isfinite(sums->sum[k])) return fail(nullptr, GSR_ERR_ARG, "gsr_surface_solve: sum %u is %g: it must be finite", k, sums->sum[k]);
    const double* s = sums->sum;
    const double inv = 1.0 / (double)sums->surface_pairs;
    double A[6][6], g[6], L[6][6] = {};
    for (int a = 0, at = 0; a < 6; a++)
        for (int b = a; b < 6; b++, at++) A[a][b] = A[b][a] = s[at];
    for (int a = 0; a < 6; a++) g[a] = -s[21 + a];
    double top = A[0][0];
    for (int a = 1; a < 6; a++) top = A[a][a] > top ? A[a][a] : top;
    const double pivot_floor = top * 0x1p-40;
    for (int j = 0; j < 6; j++) {
        double v = A[j][j];
        for (int k = 0; k < j; k++) v = v - L[j][k] * L[j][k];
        if (!(v > pivot_floor)) {
            *degenerate = j + 1;
            std::memcpy(D, IDENTITY, sizeof IDENTITY);
            return GSR_OK;
        }
        L[j][j] = std::sqrt(v);
        for (int i = j + 1; i < 6; i++) {
            v = A[i][j];
            for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[6], x[6];
    for (int i = 0; i < 6; i++) {
        double v = g[i];
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < 6; k++) v = v - L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    double w = 1.0, qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2];
    const double len = std::sqrt(((w * w + qx * qx) + qy * qy) + qz * qz);
    w = w / len; qx = qx / len; qy = qy / len; qz = qz / len;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[0][1] = 2.0 * (qx * qy - qz * w); R[0][2] = 2.0 * (qx * qz + qy * w);
    R[1][0] = 2.0 * (qx * qy + qz * w); R[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz); R[1][2] = 2.0 * (qy * qz - qx * w);
    R[2][0] = 2.0 * (qx * qz - qy * w); R[2][1] = 2.0 * (qy * qz + qx * w); R[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
    for (int k = 0; k < 3; k++) {
        D[4 * k + 0] = R[k][0]; D[4 * k + 1] = R[k][1]; D[4 * k + 2] = R[k][2];
        D[4 * k + 3] = x[3 + k];
    }
    if (rms) *rms = std::sqrt(s[27] * inv);
    *degenerate = 0;
    return GSR_OK;
}

// Horn's closed form on the sums, in the header's written order.  f64; no context, no device.
int gsr_rigid_solve(const gsr_match_sums* sums, double* D, double* rms)
{
    if (!sums || !D) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_solve: a NULL pointer");
    if (sums->pairs < 3u) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_solve: %llu pairs: at least 3 are needed", (unsigned long long)sums->pairs);
    for (uint32_t k = 0; k < MATCH_ROW; k++)
        if (!std::isfinite(sums->sum[k])) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_solve: sum %u is %g: it must be finite", k, sums->sum[k]);
    const double* s = sums->sum;
    const double inv = 1.0 / (double)sums->pairs;
    double mT[3], mQ[3], S[3][3];
    for (int a = 0; a < 3; a++) { mT[a] = s[a] * inv; mQ[a] = s[3 + a] * inv; }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) S[a][b] = s[6 + 3 * a + b] * inv - mT[a] * mQ[b];
    double A[4][4], V[4][4];
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    A[0][1] = S[1][2] - S[2][1];
    A[0][2] = S[2][0] - S[0][2];
    A[0][3] = S[0][1] - S[1][0];
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    A[1][2] = S[0][1] + S[1][0];
    A[1][3] = S[2][0] + S[0][2];
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    A[2][3] = S[1][2] + S[2][1];
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < 4; q++) { if (q < p) A[p][q] = A[q][p]; V[p][q] = p == q ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 8; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double app = A[p][p], aqq = A[q][q];
                const double th = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (std::fabs(th) + std::sqrt(th * th + 1.0));
                if (th < 0.0) t = -t;
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                A[p][p] = app - t * apq;
                A[q][q] = aqq + t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int r = 0; r < 4; r++) {
                    if (r == p || r == q) continue;
                    const double arp = A[r][p], arq = A[r][q];
                    A[r][p] = A[p][r] = cs * arp - sn * arq;
                    A[r][q] = A[q][r] = sn * arp + cs * arq;
                }
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = cs * vkp - sn * vkq;
                    V[k][q] = sn * vkp + cs * vkq;
                }
            }
    int best = 0;
    for (int k = 1; k < 4; k++) if (A[k][k] > A[best][best]) best = k;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double len = std::sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / len; x = x / len; y = y / len; z = z / len;
    const double first = w != 0.0 ? w : x != 0.0 ? x : y != 0.0 ? y : z;
    if (first < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z); R[0][1] = 2.0 * (x * y - z * w); R[0][2] = 2.0 * (x * z + y * w);
    R[1][0] = 2.0 * (x * y + z * w); R[1][1] = 1.0 - 2.0 * (x * x + z * z); R[1][2] = 2.0 * (y * z - x * w);
    R[2][0] = 2.0 * (x * z - y * w); R[2][1] = 2.0 * (y * z + x * w); R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    for (int k = 0; k < 3; k++) {
        D[4 * k + 0] = R[k][0]; D[4 * k + 1] = R[k][1]; D[4 * k + 2] = R[k][2];
        D[4 * k + 3] = mQ[k] - ((R[k][0] * mT[0] + R[k][1] * mT[1]) + R[k][2] * mT[2]);
    }
    if (rms) *rms = std::sqrt(s[15] * inv);
    return GSR_OK;
}

// out = D o M: apply M, then D.  out may be D or M.
int gsr_rigid_compose(const double* D, const double* M, double* out)
{
    if (!D || !M || !out) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_compose: a NULL pointer");
    double r[12];
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 4; c++) {
            double v = (D[4 * k + 0] * M[c] + D[4 * k + 1] * M[4 + c]) + D[4 * k + 2] * M[8 + c];
            if (c == 3) v = v + D[4 * k + 3];
            r[4 * k + c] = v;
        }
    std::memcpy(out, r, sizeof r);
    return GSR_OK;
}

// (x, y, z, w) of M's 3 x 3 part by Shepperd's four branches (the header's "merging cells", step 9), and its translation
int gsr_rigid_decompose(const double* M, double* q, double* t)
{
    if (!M || !q || !t) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_decompose: a NULL pointer");
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(M[k])) return fail(nullptr, GSR_ERR_ARG, "gsr_rigid_decompose: entry %d is %g: it must be finite", k, M[k]);
    const double R00 = M[0], R01 = M[1], R02 = M[2], R10 = M[4], R11 = M[5], R12 = M[6], R20 = M[8], R21 = M[9], R22 = M[10];
    const double tr = (R00 + R11) + R22;
    double x, y, z, w;
    if (tr > 0.0) {
        const double s = std::sqrt(tr + 1.0) * 2.0;
        w = 0.25 * s; x = (R21 - R12) / s; y = (R02 - R20) / s; z = (R10 - R01) / s;
    } else if (R00 > R11 && R00 > R22) {
        const double s = std::sqrt(((1.0 + R00) - R11) - R22) * 2.0;
        w = (R21 - R12) / s; x = 0.25 * s; y = (R01 + R10) / s; z = (R02 + R20) / s;
    } else if (R11 > R22) {
        const double s = std::sqrt(((1.0 + R11) - R00) - R22) * 2.0;
        w = (R02 - R20) / s; x = (R01 + R10) / s; y = 0.25 * s; z = (R12 + R21) / s;
    } else {
        const double s = std::sqrt(((1.0 + R22) - R00) - R11) * 2.0;
        w = (R10 - R01) / s; x = (R02 + R20) / s; y = (R12 + R21) / s; z = 0.25 * s;
    }
    q[0] = x; q[1] = y; q[2] = z; q[3] = w;
    t[0] = M[3]; t[1] = M[7]; t[2] = M[11];
    return GSR_OK;
}

// Eight floats of the context's last call, between events on the stream: index_ms (the target's index, built once per call); bound_ms,
// walk_ms and tree_ms of its last step; the sums of those three over its steps; the steps.  Not part of the ABI (tools/bench_cabi.cpp
// --register).
int gsr_debug_match_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    std::memcpy(out, c->mt.ms, sizeof c->mt.ms);
    return GSR_OK;
}

// the bytes of device scratch the context holds for these calls beside the neighbour scratch: 0 until the first call.  Not part
// of the ABI (tests/test_gpu_match.py).
int gsr_debug_match_scratch(gsr_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return GSR_ERR_ARG;
    const gsr_ctx::Match& mt = c->mt;
    *bytes = (mt.words ? MATCH_INFO_WORDS * 4ull : 0ull) + (uint64_t)mt.rows * 12u + mt.tree_rows * MATCH_ROW * 8u + mt.surface_rows * MATCH_SURFACE_ROW * 8u;
    return GSR_OK;
}

}  // extern "C"
