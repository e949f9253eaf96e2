// Merging cells: voxel simplification of the scene (include/gsplat_hip.h, "merging cells"; kernels: k_merge.hip over
// k_neighbours.hip's index).  gsr_cells is the read-only report: it is blocking, stateless and ordered like gsr_neighbours -- it
// waits for every member's stream of a shared scene first, indexes the scene as it is now, reads it and writes none of it.
// gsr_scene_merge_cells is the edit that does exactly what the report announced: the same candidates, cells and walk, then every
// cell of two or more members reduced into its leader's row in place, and the other members removed by scene_compact, the
// compaction of gsr_scene_erase_selected (gsr_scene.cpp), which carries the hidden set and, for this call, the set of merged rows
// that becomes the selection.
// The scratch is the context's neighbour scratch (gsr_neighbours.cpp), 4 bytes per 32 splats and 12 bytes per splat of its own
// for the report, and 10 bytes per splat and three more masks for the edit; the first call allocates it, it only grows, the
// context's end frees it.  A context that never calls these allocates and launches nothing.
//
// The work budget is the neighbour budget: a walk visits one bucket per entry, the bound is the sum of the buckets' squared
// populations, and a call above its budget is refused before the walk is launched.
#include "gsr_ctx.h"

#include <cmath>
#include <cstring>

using namespace gsr;

namespace {

static_assert(sizeof(MgInfo) == MG_INFO_WORDS * 4, "MgInfo fills its words");
static_assert(MG_NONE == GSR_CELL_NONE, "the header's word");
static_assert(sizeof(gsr_cell_info) == 48, "the header's layout");

// The refusals of both calls, in the header's order.  Nothing is touched by a refused call.
int mg_check(gsr_ctx* c, const char* who, double cell, uint32_t cap, uint32_t scope, uint64_t budget)
{
    if (!(std::isfinite(cell) && cell > 0.0)) return fail(c, GSR_ERR_ARG, "%s: cell (%g) must be finite and > 0", who, cell);
    if (!std::isnormal(1.0 / cell)) return fail(c, GSR_ERR_ARG, "%s: cell (%g): 1 / cell must be finite and normal", who, cell);
    if (cap < 1u || cap > GSR_NEIGHBOUR_MAX_CAP) return fail(c, GSR_ERR_ARG, "%s: cap (%u) must be in 1 .. %u", who, cap, GSR_NEIGHBOUR_MAX_CAP);
    return scope_check(c, who, scope, budget);
}

// the context's scratch for n splats, with the edit's share when `edit`: allocated by the first call, only ever grown
int mg_ensure(gsr_ctx* c, uint32_t n, bool edit)
{
    gsr_ctx::Merge& mg = c->mg;
    const uint32_t words = fold_words(n);
    int r;
    if (!mg.words) { if ((r = mg.words.alloc(c, MG_INFO_WORDS))) return r; }
    if (mg.rows < n || mg.mask_words < words || !mg.cand) {
        mg.rows = mg.mask_words = 0;
        if ((r = mg.cand.alloc(c, words)) || (r = mg.leader.alloc(c, n)) || (r = mg.count.alloc(c, n)) || (r = mg.rank.alloc(c, n))) return r;
        mg.rows = n; mg.mask_words = words;
    }
    if (edit && (mg.edit_rows < n || mg.edit_words < words || !mg.member)) {
        mg.edit_rows = mg.edit_words = 0;
        if ((r = mg.slice.alloc(c, n)) || (r = mg.member.alloc(c, n)) || (r = mg.cells.alloc(c, (size_t)n / 2u + 1u)) || (r = mg.remove.alloc(c, words)) ||
            (r = mg.merged.alloc(c, words)) || (r = mg.carried.alloc(c, words)))
            return r;
        mg.edit_rows = n; mg.edit_words = words;
    }
    return GSR_OK;
}

gsr_cell_info mg_zero_info(uint32_t n, uint64_t budget)
{
    gsr_cell_info z{};
    z.rows_after = n;
    z.budget = budget;
    return z;
}

struct MgCall {
    MgArrays a;
    uint32_t* hist;   // the device counters, cap + 1
};

// Everything both calls share: the candidate mask, the index over it, the bound against the budget, the walk, and *info, final on
// the device and waited for.  GSR_ERR_ARG (with *info filled as far as it is known) for a bound above the budget: no walk has been
// launched.  n >= 1; the device is current and no member's stream holds work.
int mg_run(gsr_ctx* c, const char* who, double cell, uint32_t cap, uint32_t scope, uint64_t budget, bool edit, MgCall* call, gsr_cell_info* info)
{
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    if (int r = mg_ensure(c, n, edit)) return r;
    gsr_ctx::Merge& mg = c->mg;
    NbIndex ix{};
    if (int r = nb_prepare(c, who, cap, 1.0 / cell, 0.0, &ix, &call->hist)) return r;
    MgArrays a{};
    a.cand = mg.cand; a.words = fold_words(n);
    a.leader = mg.leader; a.count = mg.count; a.rank = mg.rank;
    if (edit) { a.slice = mg.slice; a.member = mg.member; a.cells = mg.cells; a.remove = mg.remove; a.merged = mg.merged; }   // (the report has none: null)
    a.info = reinterpret_cast<MgInfo*>(mg.words.p);
    call->a = a;
    const SceneDev scene = sc.arr.view();
    HIP_TRY(c, hipMemsetAsync(mg.words, 0, MG_INFO_WORDS * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(mg.leader, 0xff, (size_t)n * 4, c->stream));   // MG_NONE and 0 for every splat the walk does not reach
    HIP_TRY(c, hipMemsetAsync(mg.count, 0, (size_t)n * 4, c->stream));
    launch_mg_candidates(scene, scene_scope(sc, scope), n, a, c->stream);
    // the index of the candidates: the mask is the scope, a grid cell is an index cell
    launch_nb_build(ix, scene.px, scene.py, scene.pz, AttrScope{ATTR_SCOPE_SELECTED, a.cand, a.words, nullptr, 0u}, n, c->cu_count, nullptr, c->stream);
    launch_mg_bound(ix, a, c->cu_count, c->stream);
    NbInfo nbi{};
    MgInfo got{};
    hipError_t e0 = hipGetLastError();
    hipError_t e1 = hipMemcpyAsync(&nbi, ix.info, sizeof nbi, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipMemcpyAsync(&got, a.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, e3, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    info->in_scope = got.in_scope; info->candidates = nbi.indexed; info->pair_bound = got.pair_bound;
    if (nbi.indexed > got.in_scope || got.in_scope > n || nbi.indexed != nbi.in_scope || nbi.nonfinite)
        return fail(c, GSR_ERR_HIP, "%s: the index holds %u entries for %u candidates of %u splats in scope", who, nbi.indexed, nbi.in_scope, got.in_scope);
    if (got.pair_bound > budget)
        return fail(c, GSR_ERR_ARG, "%s: the walk would make up to %llu key tests, above the budget of %llu (cell %g puts too many splats into one bucket)", who,
                    (unsigned long long)got.pair_bound, (unsigned long long)budget, cell);
    launch_mg_walk(ix, nbi.indexed, n, cap, a, edit ? nullptr : call->hist, c->cu_count, c->stream);   // (the edit reads no histogram)
    e0 = hipGetLastError();
    e1 = hipMemcpyAsync(&got, a.info, sizeof got, hipMemcpyDeviceToHost, c->stream);
    e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2, hipGetLastError()})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
    if (got.merged_members > nbi.indexed || got.merged_cells > got.merged_members / 2u || got.cells > nbi.indexed || got.fault)
        return fail(c, GSR_ERR_HIP, "%s: %u merged cells of %u members among %u candidates", who, got.merged_cells, got.merged_members, nbi.indexed);
    info->cells = got.cells; info->merged_cells = got.merged_cells; info->merged_members = got.merged_members; info->largest = got.largest;
    info->rows_after = n - got.merged_members + got.merged_cells;
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_cells(gsr_ctx* c, double cell, uint32_t cap, uint32_t scope, uint64_t budget, uint32_t* leader, uint32_t n, uint32_t* hist, gsr_cell_info* info)
{
    if (!c) return GSR_ERR_ARG;
    if (int r = mg_check(c, "gsr_cells", cell, cap, scope, budget)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    if (leader && n != sc.n) return fail(c, GSR_ERR_ARG, "gsr_cells: n (%u) is not the scene's count (%u)", n, sc.n);
    if (sc.n) { if (int r = require_rows(c)) return r; }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_cell_info got = mg_zero_info(sc.n, budget);
    if (!sc.n) {
        if (hist) std::memset(hist, 0, (size_t)(cap + 1u) * 4);
        if (info) *info = got;
        return GSR_OK;
    }
    MgCall call;
    const int r = mg_run(c, "gsr_cells", cell, cap, scope, budget, false, &call, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    hipError_t e0 = leader ? hipMemcpyAsync(leader, call.a.leader, (size_t)sc.n * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e1 = hist ? hipMemcpyAsync(hist, call.hist, (size_t)(cap + 1u) * 4, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    hipError_t e2 = hipStreamSynchronize(c->stream);
    for (hipError_t e : {e0, e1, e2})
        if (e != hipSuccess) return fail(c, GSR_ERR_HIP, "gsr_cells failed: %s", hipGetErrorString(e));
    return GSR_OK;
}

int gsr_scene_merge_cells(gsr_ctx* c, double cell, uint32_t scope, uint64_t budget, uint32_t* new_count, gsr_cell_info* info)
{
    if (!c) return GSR_ERR_ARG;
    const char* who = "gsr_scene_merge_cells";
    if (int r = mg_check(c, who, cell, 1u, scope, budget)) return r;
    if (!budget) budget = GSR_NEIGHBOUR_DEFAULT_BUDGET;
    SharedScene& sc = *c->scene;
    const uint32_t n = sc.n;
    if (n) { if (int r = require_rows(c)) return r; }
    if (sc.sh_count) return fail(c, GSR_ERR_ARG, "%s: the scene has %u SH rows: the SH colour of a mixture is not defined", who, sc.sh_count);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = settle_members(c)) return r;
    gsr_cell_info got = mg_zero_info(n, budget);
    if (!n) {
        if (new_count) *new_count = 0;
        if (info) *info = got;
        return GSR_OK;
    }
    MgCall call;
    int r = mg_run(c, who, cell, 1u, scope, budget, true, &call, &got);
    if (info && (r == GSR_OK || r == GSR_ERR_ARG)) *info = got;
    if (r) return r;
    // nothing to merge: nothing changes, the last frame and the selection stay as they are
    if (!got.merged_cells) {
        if (new_count) *new_count = n;
        return GSR_OK;
    }
    // From here on the scene changes.  The merged rows are written where their leaders are, in place: every cell reads its own
    // members only, and nothing of any member is in flight (settle_members).  The compaction then drops the other members.
    gsr_ctx::Merge& mg = c->mg;
    const MgArrays& a = call.a;
    HIP_TRY(c, hipMemsetAsync(mg.carried, 0, (size_t)a.words * 4, c->stream));
    launch_mg_members(n, got.merged_members, a, c->stream);
    launch_mg_reduce(sc.arr.view(), n, got.merged_cells, got.merged_members, a, c->stream);
    HIP_TRY(c, hipGetLastError());
    uint32_t kept = 0;
    const SetCarry carry{a.merged, a.words, mg.carried, a.words};
    if ((r = scene_compact(c, ScenePred{nullptr, a.remove, 0u, a.words}, who, &kept, &carry))) return r;
    uint32_t fault = 0;
    HIP_TRY(c, hipMemcpyAsync(&fault, &a.info->fault, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (fault || kept != got.rows_after) return fail(c, GSR_ERR_HIP, "%s: %u rows are left where %u were announced (%u faults)", who, kept, got.rows_after, fault);
    // the selection becomes exactly the merged rows (the compaction left the empty one): the carried set, folded in as every picker folds
    if ((r = select_ensure(c))) return r;
    SharedScene::Selection& sel = sc.sel;
    HIP_TRY(c, hipMemcpyAsync(sel.scratch, mg.carried, (size_t)std::min(sel.words, a.words) * 4, hipMemcpyDeviceToDevice, c->stream));
    if ((r = select_fold_and_count(c, SELOP_REPLACE, nullptr))) return r;
    if (new_count) *new_count = kept;
    return GSR_OK;
}

// the bytes of device scratch the context holds for these calls beside the neighbour scratch: 0 until the first call.  Not part
// of the ABI (tests/test_gpu_merge.py).
int gsr_debug_merge_scratch(gsr_ctx* c, uint64_t* bytes)
{
    if (!c || !bytes) return GSR_ERR_ARG;
    const gsr_ctx::Merge& mg = c->mg;
    *bytes = (mg.words ? MG_INFO_WORDS * 4ull : 0ull) + (uint64_t)mg.mask_words * 4u + (uint64_t)mg.rows * 12u + (uint64_t)mg.edit_rows * 8u +
             (mg.edit_rows ? ((uint64_t)mg.edit_rows / 2u + 1u) * 8u : 0ull) + (uint64_t)mg.edit_words * 12u;
    return GSR_OK;
}

}  // extern "C"
