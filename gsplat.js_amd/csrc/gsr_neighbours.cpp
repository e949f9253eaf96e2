// Neighbours: for every splat in scope the number of other splats in scope within a radius, capped -- the count itself, its
// histogram, and the splats whose count lies in a range as a picker (include/gsplat_hip.h, "neighbours"; kernels: k_neighbours.hip).
// Both calls are blocking, stateless and ordered like gsr_select_attr: they wait for every member's stream of a shared scene first,
// index the scene as it is now, read it and write none of it; gsr_select_neighbours changes the selection the way every picker
// does.  The scratch -- the hashed grid, the counts, the call's words and histogram counters -- is the context's: the first call
// allocates it, it only grows, the context's end frees it.  A context that never calls these allocates and launches nothing.
//
// The work budget.  A radius that puts the whole scene into one cell makes the count pass an O(n^2) kernel on a shared machine.
// So the index is built first, k_nb_bound sums what the count pass would walk at most, and a call whose bound lies above its
// budget is refused before the count pass is launched.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>

using namespace gsr;

namespace {

constexpr uint32_t NB_INFO_WORDS = 8;                 // NbInfo in whole 16 bytes: the histogram counters follow
static_assert(sizeof(NbInfo) <= NB_INFO_WORDS * 4, "NbInfo fits its words");
static_assert(NB_MAX_CAP == GSR_NEIGHBOUR_MAX_CAP, "the header's cap");
constexpr uint32_t NB_MAX_ROWS = 1u << 29;            // twice as many buckets still index with 32 bits

}  // namespace

// The refusals every call over the index shares, in the header's order.  Nothing is touched by a refused call.
int gsr::nb_check(gsr_ctx* c, const char* who, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t cap_min, const char* cap_name,
                  uint32_t cap_max)
{
    if (!(std::isfinite(radius) && radius > 0.0)) return fail(c, GSR_ERR_ARG, "%s: radius (%g) must be finite and > 0", who, radius);
    const double r2 = radius * radius, inv = 1.0 / radius, inv_h = 1.0 / (radius * (1.0 + 1.0 / 1024.0));
    if (!(std::isnormal(r2) && std::isnormal(inv) && std::isnormal(inv_h)))
        return fail(c, GSR_ERR_ARG, "%s: radius (%g): radius * radius and 1 / radius must be finite and normal", who, radius);
    if (cap < cap_min || cap > cap_max) return fail(c, GSR_ERR_ARG, "%s: %s (%u) must be in %u .. %u", who, cap_name, cap, cap_min, cap_max);
    return scope_check(c, who, scope, budget);
}

namespace {

// the context's scratch for n splats: allocated by the first call, only ever grown
int nb_ensure(gsr_ctx* c, uint32_t n, uint64_t buckets)
{
    gsr_ctx::Neighbours& nb = c->nb;
    if (!nb.words) { if (int r = nb.words.alloc(c, NB_INFO_WORDS + NB_MAX_CAP + 1u)) return r; }
    if (nb.rows < n || !nb.entry) {
        nb.rows = 0;
        int r;
        if ((r = nb.entry.alloc(c, n)) || (r = nb.key.alloc(c, n)) || (r = nb.counts.alloc(c, n))) return r;
        nb.rows = n;
    }
    if (nb.buckets < buckets || !nb.table) {
        nb.buckets = 0;
        if (int r = nb.table.alloc(c, (size_t)buckets * 2u)) return r;
        nb.buckets = buckets;
    }
    for (hipEvent_t& e : nb.ev) if (!e) HIP_TRY(c, hipEventCreate(&e));
    return GSR_OK;
}

}  // namespace

// nb_prepare_rows: the scratch for n rows (the scene's, or those of another scene that gsr_match.cpp indexes), the index's
// description and its zeroed words and table; nb_prepare: the same for the context's own scene.  nb_index: on top of it,
// everything up to the count pass: the index, its bound against the budget, *info.  GSR_ERR_ARG (with *info filled) when the
// bound is above the budget: no count kernel has been launched.  n >= 1; the device is current and no member's stream holds work.
int gsr::nb_prepare(gsr_ctx* c, const char* who, uint32_t cap, double inv_h, double r2, NbIndex* ix, uint32_t** hist)
{
    return nb_prepare_rows(c, who, c->scene->n, cap, inv_h, r2, ix, hist);
}

int gsr::nb_prepare_rows(gsr_ctx* c, const char* who, uint32_t n, uint32_t cap, double inv_h, double r2, NbIndex* ix, uint32_t** hist)
{
    if (n > NB_MAX_ROWS) return fail(c, GSR_ERR_ARG, "%s: the scene has %u splats; at most %u are indexed", who, n, NB_MAX_ROWS);
    uint64_t buckets = 256;   // a power of two, a multiple of k_nb_offsets' workgroup, at least twice the splats
    while (buckets < 2ull * n) buckets <<= 1;
    if (int r = nb_ensure(c, n, buckets)) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    *hist = nb.words + NB_INFO_WORDS;
    *ix = NbIndex{nb.table, (uint32_t)(buckets - 1u), nb.entry, nb.key, reinterpret_cast<NbInfo*>(nb.words.p), inv_h, r2};
    HIP_TRY(c, hipMemsetAsync(nb.words, 0, (size_t)(NB_INFO_WORDS + cap + 1u) * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(nb.table, 0, (size_t)buckets * 8, c->stream));
    return GSR_OK;
}

int gsr::nb_index(gsr_ctx* c, const char* who, double radius, uint32_t cap, uint32_t scope, uint64_t budget, bool want_hist, NbCall* call, gsr_neighbour_info* info)
{
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    NbCall k{};
    uint32_t* hist = nullptr;
    if (int r = nb_prepare(c, who, cap, 1.0 / (radius * (1.0 + 1.0 / 1024.0)), radius * radius, &k.ix, &hist)) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    k.sc = scene_scope(sc, scope);
    k.n = n;
    k.hist = want_hist ? hist : nullptr;
    HIP_TRY(c, hipMemsetAsync(nb.counts, 0, (size_t)n * 4, c->stream));
    HIP_TRY(c, hipEventRecord(nb.ev[0], c->stream));
    launch_nb_build(k.ix, sc.arr.px, sc.arr.py, sc.arr.pz, k.sc, n, c->cu_count, k.hist, c->stream);
    launch_nb_bound(k.ix, n, c->cu_count, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(nb.ev[1], c->stream);
    NbInfo got{};
    hipError_t e2 = hipMemcpyAsync(&got, k.ix.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    k.indexed = got.indexed;
    info->in_scope = got.in_scope; info->nonfinite = got.nonfinite; info->pair_bound = got.pair_bound; info->budget = budget;
    *call = k;
    if (got.indexed > n || got.indexed != got.in_scope - got.nonfinite)
        return fail(c, GSR_ERR_HIP, "%s: the index holds %u entries for %u splats in scope, %u of them non-finite", who, got.indexed, got.in_scope, got.nonfinite);
    if (got.pair_bound > budget)
        return fail(c, GSR_ERR_ARG, "%s: the count pass would make up to %llu pair tests, above the budget of %llu (radius %g puts too many splats into one cell)",
                    who, (unsigned long long)got.pair_bound, (unsigned long long)budget, radius);
    return GSR_OK;
}

namespace {

// the two stages' times of a call that ran both, by the events around them (bench_cabi --neighbours)
void nb_times(gsr_ctx* c)
{
    gsr_ctx::Neighbours& nb = c->nb;
    float a = 0.0f, b = 0.0f;
    if (hipEventElapsedTime(&a, nb.ev[0], nb.ev[1]) == hipSuccess && hipEventElapsedTime(&b, nb.ev[1], nb.ev[2]) == hipSuccess) { nb.build_ms = a; nb.count_ms = b; }
    else (void)hipGetLastError();
}

}  // namespace

extern "C" {

int gsr_neighbours(gsr_ctx* c, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t* counts, uint32_t n, uint32_t* hist,
                   gsr_neighbour_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = nb_check(c, "gsr_neighbours", radius, cap, scope, budget)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if (counts && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_neighbours: n (%u) is not the scene's count (%u)", n, sc.n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_neighbour_info got{0u, 0u, 0ull, budget};
    if (!sc.n) {
        if (hist) std::memset(hist, 0, (size_t)(cap + 1u) * 4);
        if (info) *info = got;
        return GSR_OK;
    }
    NbCall k;
    const int r = nb_index(c, "gsr_neighbours", radius, cap, scope, budget, hist != nullptr, &k, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    launch_nb_count(k.ix, k.indexed, k.n, cap, nb.counts, k.hist, c->cu_count, c->stream);
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipEventRecord(nb.ev[2], c->stream);
    hipError_t e2 = counts ? hipMemcpyAsync(counts, nb.counts, (size_t)k.n * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e3 = hist ? hipMemcpyAsync(hist, k.hist, (size_t)(cap + 1u) * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e4 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, e4, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_neighbours failed: %s", hipGetErrorString(e));
    nb_times(c);
    return GSR_OK;
}

int gsr_select_neighbours(gsr_ctx* c, double radius, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t lo, uint32_t hi, int32_t op,
                          uint32_t* selected, gsr_neighbour_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = nb_check(c, "gsr_select_neighbours", radius, cap, scope, budget)) return r;
    if (!op_ok(op)) return fail(c, GSR_ERR_ARG, "gsr_select_neighbours: unknown op %d", op);
    if (lo > hi || hi > cap + 1u) return fail(c, GSR_ERR_ARG, "gsr_select_neighbours: [%u, %u) must satisfy lo <= hi <= cap + 1 = %u", lo, hi, cap + 1u);
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    SharedScene& sc = *c->scene;
    gsr_neighbour_info got{0u, 0u, 0ull, budget};
    if (!sc.n) {
        if (selected) *selected = 0;
        if (info) *info = got;
        return GSR_OK;
    }
    if (int r = select_ensure(c)) return r;   // (in front of the scope: a selection never allocated becomes the zeroed mask, the same set)
    NbCall k;
    const int r = nb_index(c, "gsr_select_neighbours", radius, cap, scope, budget, false, &k, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    gsr_ctx::Neighbours& nb = c->nb;
    launch_nb_count(k.ix, k.indexed, k.n, cap, nb.counts, nullptr, c->cu_count, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(nb.ev[2], c->stream));
    launch_nb_select(nb.counts, k.sc, k.n, lo, hi, sc.sel.scratch, sc.sel.words, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (int r2 = select_fold_and_count(c, op, selected)) return r2;
    nb_times(c);
    return GSR_OK;
}

// (build_ms, count_ms) of the context's last call that ran both stages: the index with its bound, and the count pass, between
// events on the stream.  Not part of the ABI (tools/bench_cabi.cpp --neighbours).
int gsr_debug_neighbour_times(gsr_ctx* c, float* out)
{
    if (!c || !out) return GSR_ERR_ARG;
    out[0] = c->nb.build_ms; out[1] = c->nb.count_ms;
    return GSR_OK;
}

}  // extern "C"
