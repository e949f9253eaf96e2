"""What a frame may depend on (State), everything a host can do to a context between frames (operations), and sequences of
them (traces): the material of tests/test_gpu_history.py, which walks one long-lived context through a trace and compares every
frame, bit for bit, with the frame of a context created a moment ago from the State alone.

Pure Python and numpy: building and folding a trace needs no GPU (tests/test_history_trace.py); only `apply` and `build`
touch a renderer.  An operation is a tuple (kind, *arguments); a trace is a list of Step(op, check): after a checked step the
test renders the State's pose on both contexts and compares, an unchecked step is followed directly by the next operation.

The editing layer -- selection, hidden set, edits of the selection, growth and erasure, overlay, contribution -- is part of the State
as a RECIPE (State.edits): `materialise` evaluates it on the CPU with the specifications the feature suites already have
(edit_reference, append_reference, hide_reference, select_reference, attr_reference over oracle.SceneState), and `build` uploads the
result, so the fresh context has a capacity equal to its count, never ran an edit kernel and never grew.  KINDS, REFUSALS, tour() and
the walks over KINDS keep their exact content (tests/test_history_trace.py pins a digest); the new operations are EDIT_KINDS and
EDIT_REFUSALS, the new fixed trace editing_tour(), the new pairs EDIT_RISKY_PAIRS, and walk(..., kinds=KINDS + EDIT_KINDS).
HIT-mode region selection stays out of the traces: its result is defined by the device's own index plane, so it has no pure fold;
tests/test_gpu_select.py covers it.  gsr_select_contrib is folded at the two thresholds whose set needs no frame (below = +inf:
every splat, below = 0: none); the accumulators themselves are compared through read_contrib().

The analysis layer -- neighbour counts, clusters, k nearest neighbours, merge cells -- joins the same way: its pickers and the merge
are entries of State.edits, evaluated by neighbour_reference, cluster_reference, knn_reference and merge_reference under scope masks
computed from the recipe's own selection and hidden set; its read-only calls are ("report", ...) operations that fold to the same
State.  ANALYSIS_KINDS, ANALYSIS_REFUSALS, analysis_tour(), ANALYSIS_RISKY_PAIRS and walk(..., kinds=KINDS + EDIT_KINDS +
ANALYSIS_KINDS) are new; editing_tour() and the walks over KINDS + EDIT_KINDS keep their exact content (a second digest pins them).
The fresh context is still uploaded from CPU-evaluated arrays and never ran an analysis kernel before its own observables: the
feature suites pin every one of these calls to its reference exactly.  No threshold is computed from device values inside a trace:
the statistical outlier filter is select_knn with a constant lower end, followed by erase."""
import os
import random
from collections import namedtuple
from dataclasses import dataclass, replace

import numpy as np

GSR_ERR_ARG, GSR_ERR_SCENE, GSR_ERR_OVERFLOW = -1, -4, -5   # include/gsplat_hip.h

Step = namedtuple("Step", "op check")


@dataclass(frozen=True)
class State:
    """Everything an observable of a frame may depend on -- and nothing else a context remembers."""
    kind: str = "default"            # "default" | "throughput": the two kinds of context bench.py and the hosts create
    timing: bool = False             # created with GSR_FLAG_TIMING
    knobs: tuple = ()                # ((environment name, value), ...): read once, when the context is created
    W: int = 640
    H: int = 480
    band: tuple = None               # (x0, x1) as the library keeps it (x1 clamped to W), None: the whole frame
    scene: tuple = ("synth", 2049, 5, "raw")   # recipe: ("synth", n, seed, form) | ("config", name, form); form "rows" | "raw"
    transforms: tuple = ()           # (("rotate" | "translate" | "scale" | "limit_box", values), ...) applied on the device, in order
    sh: tuple = None                 # (seed, f0, f1, f2): half textures from `seed`, band indices at those fractions of the count
    fade: tuple = (False, 0.0)       # (use, value) of gsr_set_depth_fade
    hit_alpha: float = 0.5
    ring: tuple = None               # (format, full_range, depth format | None, depth step): the open delivery ring
    pose: int = 0                    # camera k of the 120-frame orbit at this size
    # the editing layer, as a recipe (materialise evaluates it on the CPU)
    edits: tuple = ()                # the ordered scene-changing operations since the scene was set: pickers, hides, edits of the selection,
    #                                  growth, erasure -- and, once there is one, the whole-scene transforms behind it (("transform", name, values))
    overlay: tuple = None            # (tint, mix, outline options (rgb, alpha, threshold, width, side) | None), None: off
    ring_overlay: bool = False       # the open ring delivers the overlay in place of the frame
    contrib: tuple = None            # the passes since the last reset, (pose, W, H, band, fade, len(edits) at the pass) each; None: never reset


# Read-backs that must not disturb anything, and calls that are refused and must change nothing.
READBACKS = ("records", "keys", "bin_lists", "work_items", "depth_index", "read_depth", "pick", "stats")
REFUSALS = ("band_off_boundary", "size_zero", "positions_differ", "timing_interval_zero")
KINDS = ("camera", "same_pose", "burst", "sort_only", "readback", "scene", "resize", "band", "sh", "limit_box", "rotate",
         "translate", "scale", "fade", "hit_alpha", "depth_async", "timing_interval", "overflow_sync", "overflow_async",
         "ring_open", "ring_close", "deliver", "refused")
# operations after which the last frame's lists, records and planes are still the context's: only these may go unchecked
# (an unchecked step is followed directly by the next operation, which may be a read-back of that frame)
KEEPS_FRAME = ("camera", "same_pose", "burst", "sort_only", "readback", "fade", "hit_alpha", "timing_interval", "deliver", "depth_async")

# The editing layer's operations (KINDS itself stays: tour() and the seeded walks over it keep their exact content).
SELECT_KINDS = ("select_box", "select_region", "set_selection", "invert_selection", "select_attr", "select_hidden", "select_contrib")
EDIT_KINDS = SELECT_KINDS + ("hide", "set_hidden", "edit", "reserve", "duplicate", "append_arrays", "erase", "overlay", "ring_overlay",
                             "contrib_reset", "contrib_pass")
# refused calls of the editing layer (REFUSALS stays as it is, like KINDS): an edit and an erase on a raw scene, growth with SH rows,
# rotate-selected with SH follow on, append_arrays whose positions differ from its data
EDIT_REFUSALS = ("edit_raw", "erase_raw", "grow_with_sh", "rotate_selected_sh_follow", "append_positions_differ")
# of the new kinds only the pickers, a contribution pass and the overlay's option calls keep the frame: edits, hides and growth invalidate it
EDIT_KEEPS_FRAME = SELECT_KINDS + ("contrib_pass", "overlay")
# operations that move splats or change which are listed while the indices stay: live accumulators then describe frames no State can
# render again, so the traces reset the accumulators in front of them (walk() does it itself)
MOVES_GEOMETRY = ("rotate", "translate", "scale", "edit")
MAX_GROWN = 40000                     # no trace grows a scene beyond this

# The analysis layer: neighbour counts, clusters, k nearest neighbours and merge cells (KINDS, EDIT_KINDS and the traces over them stay).
# The four pickers join State.edits like select_attr and keep the frame; merge_cells is an edit that removes rows from the inside;
# ("report", which, ...) are the read-only calls gsr_neighbours / gsr_clusters / gsr_knn / gsr_cells.  Operations:
#   ("select_neighbours", radius, lo, hi, cap, scope, op)          ("select_clusters", radius, lo, hi, min_pts, scope, op)
#   ("select_cluster_at", radius, seed, min_pts, scope, op)        ("select_knn", radius, k, stat, lo, hi, scope, op)
#   ("merge_cells", cell, scope)
#   ("report", "neighbours", radius, cap, scope) | ("report", "clusters", radius, min_pts, scope) | ("report", "knn", radius, k, stat, scope)
#       | ("report", "cells", cell, cap, scope)
# scope: a tuple of "selected" / "visible"; hi None: no upper end; seed: an index or "largest".
ANALYSIS_PICKERS = ("select_neighbours", "select_clusters", "select_cluster_at", "select_knn")
ANALYSIS_KINDS = ANALYSIS_PICKERS + ("merge_cells", "report")
REPORTS = ("neighbours", "clusters", "knn", "cells")
SCOPES = ((), ("selected",), ("visible",), ("selected", "visible"))
ANALYSIS_KEEPS_FRAME = ANALYSIS_PICKERS + ("report",)
# refused calls of the analysis layer, and a piece of the message each must carry (the library's texts: gsr_merge.cpp, gsr_neighbours.cpp,
# gsr_scene.cpp).  budget_of_one is the first picker, gsr_select_neighbours, with a budget of 1: refused before any walk, selection untouched.
ANALYSIS_REFUSAL_TEXTS = {
    "merge_raw": "need a scene built with gsr_set_scene_rows or gsr_set_scene_arrays",
    "merge_with_sh": "SH rows: the SH colour of a mixture is not defined",
    "budget_of_one": "above the budget of 1 (radius",
    "cell_not_finite": "gsr_scene_merge_cells: cell (inf) must be finite and > 0",
    "cell_not_positive": "gsr_cells: cell (0) must be finite and > 0",
    "radius_not_finite": "gsr_select_knn: radius (nan) must be finite and > 0",
    "radius_not_positive": "gsr_select_clusters: radius (-0.25) must be finite and > 0",
    "cap_out_of_range": "gsr_select_neighbours: cap (4096) must be in 1 .. 4095",
    "k_out_of_range": "gsr_knn: k (33) must be in 1 .. 32",
}
ANALYSIS_REFUSALS = tuple(ANALYSIS_REFUSAL_TEXTS)
MAX_ANALYSED = 8192                   # the references are blocked brute force: no trace holds an analysis operation on a larger scene

# Ordered pairs of neighbours the tour must visit (tags as `tags` gives them), and why each is risky.
RISKY_PAIRS = (
    ("band:on", "band:off", "the full frame indexes rect[] / depth[] by splat where the band frame wrote survivors only"),
    ("band:off", "band:on", "the earlier band again: culled splats still hold the full frame's rectangles, packed slots its depths"),
    ("band:on", "band:move", "a splat culled now was a survivor a frame ago and keeps that rectangle"),
    ("band:on", "resize", "gsr_resize drops the band without a gsr_set_band: the planes' fill key and the survivor buffers stay"),
    ("sort_only", "resize", "the sort-only frames' slot sets and parity meet a new bin grid"),
    ("sort_only", "readback", "a read-back directly behind a sort-only frame reads the render frame's buffers, not the sort's"),
    ("sort_only", "scene", "the slot set the last k_depth_key reset belongs to a scene that is gone"),
    ("scene:empty", "sort_only", "the parity does not move on an empty scene: the same slot set twice"),
    ("overflow_sync", "scene", "a regrown list, then gsr_set_scene sets the capacity back to 'by the scene'"),
    ("overflow_async", "scene", "dropped frames and a sticky device counter, then every per-splat buffer is new"),
    ("overflow_async", "band:on", "max_items was reset by the regrowth; the band's grid sizes the items anew"),
    ("readback:records", "camera", "k_project_key ran a second time over the render frames' slot set and the live rec / rect buffers"),
    ("readback:records", "same_pose", "... and the next frame is a graph replay with nothing rewritten but the camera"),
    ("burst", "readback:keys", "three frames in flight, then the keys of the last one"),
    ("sh:on", "limit_box", "the compaction renumbers the splats: SH rows and shcol[] of the old numbering must go"),
    ("limit_box", "sh:on", "SH for a scene whose count shrank while every per-splat buffer kept its size"),
    ("sh:on", "sh:off", "rgb8 records again after RGB8_IN_SHCOL ones"),
    ("scene:shrink", "camera", "buffers sized for the larger scene: the tail of depth[] / keys / rect[] is the old scene's"),
    ("scene:grow", "camera", "every per-splat buffer is new, the bin table may not be"),
    ("scene:rows", "scene:raw", "rotations / scales are dropped; transforms are refused from here on"),
    ("scene:raw", "scene:rows", "and allocated again"),
    ("resize:shrink", "resize:grow", "the original size again: framebuffer, planes and per-bin arrays were never shrunk"),
    ("ring_open", "resize", "the ring is reallocated at the new size and keeps its format"),
    ("resize", "deliver", "the first delivery into the new blocks"),
    ("ring_close", "ring_open", "another format in the slots' place"),
    ("hit_alpha", "depth_async", "planes cached for a frame_serial were cut at the old threshold"),
    ("depth_async", "camera", "the planes on the device belong to the frame before"),
    ("timing_interval", "camera", "individual launches with events, then graph replays, alternating"),
    ("fade:on", "fade:off", "the fade is part of the camera argument of the one node a replay rewrites"),
    ("refused", "camera", "a call that failed must have changed nothing the next frame reads"),
)

# The same for the editing layer (editing_tour visits them).  Tags: "select" for every picker, "hide:on" for a hide that adds or
# replaces, "hide:off" for show-all, "duplicate:fit" / "duplicate:grow" for a duplicate inside / beyond the capacity, "overlay:on" / ":off".
EDIT_RISKY_PAIRS = (
    ("hide:on", "same_pose", "the hidden mask arrives in FrameArgs: the graph captured without it must not be replayed"),
    ("hide:on", "hide:off", "the null pointer returns while the buffers stay allocated, and the graph is dropped again"),
    ("hide:on", "band:on", "a hidden splat is no survivor: the pack path of k_project_key reads the mask"),
    ("band:on", "hide:on", "survivor slots and rectangles of the frame before belong to splats that are hidden now"),
    ("hide:on", "overflow_sync", "the frame rendered again by the repair must hide what the first attempt hid"),
    ("hide:on", "overflow_async", "dropped frames, regrown lists, and a mask that arrived between captures"),
    ("hide:on", "sort_only", "gsr_sort does not look at the mask: the render frame behind it must"),
    ("hide:on", "scene", "gsr_set_scene* leaves nothing hidden: the pointer is null again though the buffers were sized for the old scene"),
    ("scene", "hide:on", "the first hide of a scene allocates the mask for this count"),
    ("hide:on", "erase", "the compaction carries H to the new numbering"),
    ("hide:on", "limit_box", "... and so does gsr_scene_limit_box, which drops the selection"),
    ("duplicate:grow", "same_pose", "the arrays are new, generation moved: a replayed graph would read the freed ones"),
    ("duplicate:fit", "same_pose", "nothing re-allocated, but n is a kernel argument of every node"),
    ("reserve", "same_pose", "capacity above n: the rows behind n are stale and the arrays moved under a captured graph"),
    ("duplicate", "burst", "three frames in flight over per-splat buffers sized a moment ago"),
    ("duplicate", "band:on", "survivor buffers sized by the old count"),
    ("duplicate", "resize", "a new bin grid and new per-splat buffers at once"),
    ("duplicate", "erase", "the compaction reads n rows of arrays that hold capacity rows"),
    ("erase", "duplicate", "the copies land on rows the compaction left stale"),
    ("duplicate:grow", "sort_only", "alloc_sort runs only when n > sort.rows: past it and past a keys-per-block multiple"),
    ("append_arrays", "limit_box", "the compaction of a scene whose tail was uploaded, not built"),
    ("edit", "same_pose", "an edit changes no argument: the replayed graph must still read the edited rows"),
    ("edit", "sort_only", "the sorted order of the frame before is marked edited"),
    ("edit", "readback:pick", "a pick behind an edit needs the new frame"),
    ("select", "limit_box", "a selection does not survive a limitBox"),
    ("select", "scene", "nor a new scene"),
    ("overlay:on", "resize", "the overlay's images follow the size"),
    ("overlay:on", "hide:on", "the pass walks this frame's lists: a hidden selected splat tints nothing"),
    ("overlay:on", "duplicate", "the selection mask grew with the capacity and holds exactly the copies"),
    ("overlay:on", "band:on", "the pass and the outline are defined on the band's columns"),
    ("ring_overlay", "deliver", "the ring converts the overlay image in place of the framebuffer"),
    ("ring_overlay", "resize", "the ring survives the resize with its overlay flag; the images are new"),
    ("ring_overlay", "overlay:off", "the switch is the ring's and stays when the options go: deliveries are refused until they return"),
    ("erase", "band:on", "a band frame behind a compaction must not read a rectangle of the old numbering"),
    ("contrib_pass", "duplicate", "the accumulators grow with zeros behind the old rows' values"),
    ("contrib_pass", "erase", "a compaction drops the accumulators: never reset again"),
    ("contrib_pass", "scene", "and so does a new scene"),
) + tuple(("refused:" + w, "camera", "a refused call of the editing layer must have changed nothing the next frame reads") for w in EDIT_REFUSALS)

# The same for the analysis layer (analysis_tour visits them).  Tags: "merge" for merge_cells, "select" and the kind for every picker,
# "report" and "report:<which>" for the read-only calls.  All four features share one neighbour scratch and one hashed index per context
# (nb_prepare / launch_nb_build, gsr_neighbours.cpp), rebuilt by each call with its own cell side; the merge's own scratch is sized by
# mg.rows and mg.edit_rows (mg_ensure, gsr_merge.cpp).
ANALYSIS_RISKY_PAIRS = (
    # merge in front of a later frame, buffer or edit
    ("merge", "same_pose", "rows were rewritten in place and compacted: the graph captured over the old count must not be replayed"),
    ("merge", "sort_only", "the sorted order of the frame before numbers rows that are gone"),
    ("merge", "burst", "three frames in flight over per-splat buffers whose tail is the old scene's"),
    ("merge", "band:on", "a band frame behind the merge must not read a rectangle or a survivor slot of the old numbering"),
    ("band:on", "merge", "survivor slots of the band frame before belong to rows the merge removes"),
    ("merge", "resize", "a new bin grid over a scene whose count just moved"),
    ("overflow_async", "merge", "dropped frames and a sticky device counter, then the rows move under the regrown lists"),
    ("burst", "merge", "the merge waits for three frames in flight before it writes their rows in place"),
    ("merge", "readback:records", "k_project_key runs a second time over the merged rows and the live rec / rect buffers"),
    ("merge", "erase", "a second compaction over the first one's stale tail, the selection being exactly the merged rows"),
    # merge and the hidden set, in both scopes
    ("hide:on", "merge", "the compaction carries H to the new numbering; under scope visible a hidden member stays out of its cell"),
    ("merge", "hide:off", "the null pointer returns behind a carried set"),
    # merge and capacity above n
    ("duplicate:grow", "merge", "the arrays are new and the copies sit exactly on their originals: every copy merges with its original"),
    ("duplicate:fit", "merge", "the merge reads n rows of arrays that hold capacity rows"),
    ("reserve", "merge", "capacity above n: the rows behind n are stale, and the scratch is sized by n"),
    ("merge", "duplicate", "the copies land on rows the merge's compaction left stale"),
    ("append_arrays", "merge", "the merge of a scene whose tail was uploaded, not built"),
    # merge and the layers that follow the selection
    ("contrib_pass", "merge", "the accumulators are dropped as a removing erase drops them: never reset again"),
    ("overlay:on", "merge", "the selection becomes the merged rows: the overlay tints exactly those"),
    ("ring_overlay", "merge", "the ring delivers the overlay of a selection the merge replaces ..."),
    ("merge", "deliver", "... and the first delivery behind it shows the merged rows"),
    # merge and the scratch sizing paths
    ("merge", "merge", "a larger cell over the rows the first merge wrote: scratch, index and carried masks of the larger count stay behind"),
    ("scene:grow", "merge", "mg.rows < n and mg.edit_rows < n: both shares of the scratch are allocated anew"),
    ("scene:shrink", "merge", "scratch larger than the scene: masks and tables of the old count behind the words in use"),
    ("report:cells", "merge", "the report grew its own share of the scratch only: the edit's share is behind (mg.edit_rows < n)"),
    # different features back to back over the one index and scratch, a different radius each time
    ("select_neighbours", "select_knn", "the index of the call before has another cell side"),
    ("select_knn", "select_clusters", "... and another"),
    ("select_clusters", "merge", "the merge indexes cells of its own side over the clusters' table"),
    ("merge", "select_neighbours", "the index of the merge holds the old numbering's entries"),
    # a picker behind a change of positions, numbering or hidden set
    ("edit", "select_neighbours", "the selected splats moved: an index kept from before would count the old places"),
    ("translate", "select_knn", "every position changed"),
    ("limit_box", "select_clusters", "the compaction renumbered the splats: labels are indices"),
    ("erase", "select_cluster_at", "the seed is an index of the new numbering"),
    ("hide:on", "select_neighbours", "under scope visible the hidden splats are no neighbours"),
) + tuple(("report:" + w, "same_pose", "a report disturbs no frame: the next one is a graph replay") for w in REPORTS) + tuple(
    ("report:" + w, "readback:bin_lists", "... and the last frame's lists are still there to be read") for w in REPORTS) + tuple(
    ("refused:" + w, "camera", "a refused call of the analysis layer must have changed nothing the next frame reads") for w in ANALYSIS_REFUSALS)


# ---------------------------------------------------------------------------------------------------------------------------
# State arithmetic (pure)
# ---------------------------------------------------------------------------------------------------------------------------
def scene_n(recipe):
    if recipe[0] == "config":
        from gsplat_hip import synth
        return synth.CONFIGS[recipe[1]]["n"]
    return recipe[1]


def scene_form(recipe):
    return recipe[-1]


def fold(state, op):
    """The State after `op` (what the library documents; the GPU tests check that the contexts agree)."""
    kind, a = op[0], op[1:]
    if kind in ("camera",):
        return replace(state, pose=a[0])
    if kind == "burst":
        return replace(state, pose=a[-1])
    if kind == "overflow_async":
        return replace(state, pose=a[-1])
    if kind == "scene":    # (selection, hidden set and accumulators are the scene's: gone with it)
        return replace(state, scene=a[0], transforms=(), sh=None, edits=(), contrib=None)
    if kind == "resize":
        return replace(state, W=a[0], H=a[1], band=None)          # (gsr_resize drops the band; ring and overlay follow the size)
    if kind == "band":
        return replace(state, band=None if a == (0, 0) else (a[0], min(a[1], state.W)))
    if kind == "sh":
        return replace(state, sh=a[0])
    if kind == "limit_box":    # (the compaction drops the SH state, the selection and the accumulators, and carries the hidden set)
        if state.edits:
            return replace(state, edits=state.edits + (("transform", kind, a[0]),), sh=None, contrib=None)
        return replace(state, transforms=state.transforms + (("limit_box", a[0]),), sh=None, contrib=None)
    if kind in ("rotate", "translate", "scale"):
        if state.edits:        # (behind an edit the order matters: the transform joins the recipe)
            return replace(state, edits=state.edits + (("transform", kind, a[0]),))
        return replace(state, transforms=state.transforms + ((kind, a[0]),))
    if kind == "fade":
        return replace(state, fade=(bool(a[0]), float(a[1])))
    if kind == "hit_alpha":
        return replace(state, hit_alpha=float(a[0]))
    if kind == "ring_open":    # (a newly opened ring delivers the frame)
        return replace(state, ring=tuple(a), ring_overlay=False)
    if kind == "ring_close":
        return replace(state, ring=None, ring_overlay=False)
    # -- the editing layer
    if kind == "select_region":    # a region picks from a frame: the op records the frame it was made under
        return replace(state, edits=state.edits + ((kind,) + a + (frame_of(state),),))
    if kind in SELECT_KINDS or kind in ("hide", "set_hidden", "edit", "append_arrays"):
        return replace(state, edits=state.edits + (op,))
    if kind == "duplicate":        # (its argument is the trace's expectation "fit" / "grow" / None, no part of the recipe)
        return replace(state, edits=state.edits + ((kind,),))
    if kind == "erase":            # (a removing erase drops the SH state and the accumulators; the traces' erases all remove)
        return replace(state, edits=state.edits + (op,), sh=None, contrib=None)
    if kind == "overlay":          # (the ring's switch is the ring's: it stays when the options go, see overlay_ring_refuses)
        return replace(state, overlay=None if a[0] is None else tuple(a))
    if kind == "ring_overlay":
        return replace(state, ring_overlay=bool(a[0]))
    if kind == "contrib_reset":
        return replace(state, contrib=())
    if kind == "contrib_pass":     # (without a prior reset the first pass resets first)
        return replace(state, contrib=(state.contrib or ()) + (frame_of(state) + (len(state.edits),),))
    # -- the analysis layer
    if kind in ANALYSIS_PICKERS:
        return replace(state, edits=state.edits + (op,))
    if kind == "merge_cells":      # (a merge that merges something drops the SH state and the accumulators, as a removing erase does; the traces' merges all merge)
        return replace(state, edits=state.edits + (op,), sh=None, contrib=None)
    assert kind in KINDS or kind in ("reserve", "report"), op
    return state      # same_pose, sort_only, readback, depth_async, timing_interval, overflow_sync, deliver, refused, reserve, report


def overlay_ring_refuses(state):
    """The one State in which a delivery is refused by design: the ring was switched to the overlay and the overlay's options were
    taken away afterwards.  The switch stays (options set again, the ring delivers the overlay again); until then
    gsr_deliver_frame_async returns GSR_ERR_ARG ("the options are off") and takes no slot."""
    return state.ring is not None and state.ring_overlay and state.overlay is None


def frame_of(state):
    """what a frame's lists depend on besides the scene: (pose, W, H, band, fade)"""
    return (state.pose, state.W, state.H, state.band, state.fade)


def fold_all(state, trace):
    for st in trace:
        state = fold(state, st.op)
    return state


def tags(op, before):
    """The names an operation goes by in RISKY_PAIRS: its kind, and kind:variant where the variant matters."""
    kind, a = op[0], op[1:]
    out = {kind}
    if kind == "band":
        out.add("band:off" if a == (0, 0) else "band:move" if before.band is not None else "band:on")
        if a != (0, 0):
            out.add("band:on")
    elif kind == "scene":
        n0, n1 = scene_n(before.scene), scene_n(a[0])
        out.add("scene:" + scene_form(a[0]))
        if n1 == 0:
            out.add("scene:empty")
        if n1 > n0:
            out.add("scene:grow")
        if n1 < n0:
            out.add("scene:shrink")
    elif kind == "resize":
        p0, p1 = before.W * before.H, a[0] * a[1]
        out.add("resize:grow" if p1 > p0 else "resize:shrink")
    elif kind == "sh":
        out.add("sh:on" if a[0] else "sh:off")
    elif kind == "fade":
        out.add("fade:on" if a[0] else "fade:off")
    elif kind in ("readback", "refused"):
        out.add(kind + ":" + a[0])
    elif kind in SELECT_KINDS:
        out.add("select")
    elif kind == "hide":
        if a[0] in ("add", "replace"):
            out.add("hide:on")
    elif kind == "set_hidden":
        if a[0] is None and a[1] == "replace":
            out.update(("hide", "hide:off"))
        elif a[0] is not None and a[1] in ("add", "replace"):
            out.update(("hide", "hide:on"))
    elif kind == "duplicate":
        if a[0]:
            out.add("duplicate:" + a[0])
    elif kind == "overlay":
        out.add("overlay:off" if a[0] is None else "overlay:on")
    elif kind in ANALYSIS_PICKERS:
        out.add("select")
    elif kind == "merge_cells":
        out.add("merge")
    elif kind == "report":
        out.add("report:" + a[0])
    return out


def pairs_in(state, trace):
    """every (tag, tag) of two neighbouring operations of the trace.  A picker that goes unchecked touches no frame and no scene
    array, and some neighbours need one between them (an erase leaves the empty selection, a duplicate needs one): the operation
    in front of such a picker also counts as the neighbour of the one behind it."""
    seen, prev, through = set(), None, None
    for st in trace:
        t = tags(st.op, state)
        for p in (prev, through):
            if p is not None:
                seen.update((x, y) for x in p for y in t)
        through = (through or prev) if (st.op[0] in SELECT_KINDS + ANALYSIS_PICKERS and not st.check) else None
        prev, state = t, fold(state, st.op)
    return seen


def into_band(state, x, y):
    """a pixel of the frame moved into the State's band (gsr_pick refuses pixels outside it)"""
    if state.band is None:
        return (x, y)
    return (state.band[0] + x % (state.band[1] - state.band[0]), y)


def bins_of(W, H, band=None):
    nbx, nby = -(-W // 32), -(-H // 32)
    if band:
        return (min(-(-band[1] // 32), nbx) - band[0] // 32) * nby
    return nbx * nby


# ---------------------------------------------------------------------------------------------------------------------------
# The recipe, evaluated on the CPU (pure: the oracle and the feature suites' specifications, no renderer)
# ---------------------------------------------------------------------------------------------------------------------------
Materialised = namedtuple("Materialised", "data positions rotations scales n selection_words hidden_words")
_mat_cache = {}
_MAT_CACHE_MAX = 24


def _refs():
    import append_reference, attr_reference, edit_reference, hide_reference, select_reference
    return edit_reference, append_reference, hide_reference, select_reference, attr_reference


def recipe_rows(recipe):
    from gsplat_hip import synth
    return synth.config_rows(recipe[1]) if recipe[0] == "config" else synth.synth_rows(recipe[1], recipe[2])


def spec_set(spec, n):
    """the host's set of a set_selection / set_hidden operation: None (the empty set) or (seed, density) -> bool[n]"""
    if spec is None:
        return np.zeros(n, dtype=bool)
    return np.random.default_rng(spec[0]).random(n) < spec[1]


def mask_of(mspec):
    """the byte mask of a select_region operation: None, or ("disc", cx, cy, radius, stride_pad) -> select_reference.disc's mask"""
    if mspec is None:
        return None
    return _refs()[3].disc(*mspec[1:])[1]


def disc_rect(mspec):
    return _refs()[3].disc(*mspec[1:])[0]


def band_columns(W, band):
    """the pixel columns of a band context's whole bins (None: the whole frame)"""
    return None if band is None else (band[0] // 32 * 32, min(-(-band[1] // 32) * 32, -(-W // 32) * 32))


def project_frame(oracle, data, frame, hidden):
    """(rec, bbox) of the ORACLE for a frame (pose, W, H, band, fade) of `data`, the members of `hidden` with the invisible box"""
    import gsplat_hip as gh
    pose, W, H, band, fade = frame
    cam = gh.orbit_camera(pose, 120, W, H, fx=0.59 * W)
    v, p, _ = cam.f32()
    rec, bbox, _ = oracle.project(data, v, p, cam.fx, cam.fy, W, H, fade=fade[1] if fade[0] else None)
    return rec, _refs()[2].hide_bbox(bbox, hidden)


def listed_in(oracle, data, frame, hidden):
    """bool[n]: the splats the frame lists"""
    _, bbox = project_frame(oracle, data, frame, hidden)
    return _refs()[3].listed(bbox, band_columns(frame[1], frame[3]))


def picked_by(oracle, st, S, H, e):
    """bool[n]: the set P a picker of the recipe picks from the scene `st` (selection S, hidden set H)"""
    er, ar, hr, sr, at = _refs()
    kind = e[0]
    if kind == "select_box":
        return sr.box_pick(st.positions, e[1])
    if kind == "select_region":
        rect, mspec, frame = e[1], e[2], e[4]
        rec, bbox = project_frame(oracle, st.data[:8 * st.n], frame, H)
        return sr.centre_pick(rec, bbox, rect, mask_of(mspec), band=band_columns(frame[1], frame[3]))
    if kind == "set_selection":
        return spec_set(e[1], st.n)
    if kind == "select_attr":
        v = at.attr_value(e[1], data=st.data[:8 * st.n], positions=st.positions, scales=st.scales, origin=e[4])
        return at.select(v, e[2], e[3])
    if kind == "select_hidden":
        return H.copy()
    if kind == "select_contrib":     # value < below over all splats: everything at +inf, nothing at 0 (values are >= 0)
        assert e[2] in (np.inf, 0.0), e
        return np.full(st.n, e[2] == np.inf)
    if kind in ANALYSIS_PICKERS:
        return analysis_pick(st, scope_mask(e[-2], S, H), e)
    raise AssertionError(e)


def _analysis_refs():
    import cluster_reference, knn_reference, merge_reference, neighbour_reference
    return neighbour_reference, cluster_reference, knn_reference, merge_reference


def scope_mask(scope, S, H):
    """bool[n]: the splats in scope -- "selected": S, "visible": not H, both: the intersection, (): every splat"""
    assert set(scope) <= {"selected", "visible"}, scope
    m = np.ones(S.size, dtype=bool)
    if "selected" in scope:
        m &= S
    if "visible" in scope:
        m &= ~H
    return m


def analysis_pick(st, mask, e):
    """bool[n]: what one of ANALYSIS_PICKERS picks from the scene `st` under the scope mask, by the feature suites' specifications"""
    nr, cr, kr, _ = _analysis_refs()
    kind, pos = e[0], st.positions[:3 * st.n]
    if kind == "select_neighbours":
        radius, lo, hi, cap = e[1:5]
        return nr.select(nr.counts(pos, radius, cap, mask), lo, cap + 1 if hi is None else hi, mask)
    if kind == "select_clusters":
        radius, lo, hi, min_pts = e[1:5]
        return cr.select(cr.Clusters(pos, radius, min_pts, mask).sizes, lo, 0xffffffff if hi is None else hi, mask)
    if kind == "select_cluster_at":
        radius, seed, min_pts = e[1:4]
        c = cr.Clusters(pos, radius, min_pts, mask)
        return cr.select_at(c.labels, cr.LARGEST if seed == "largest" else seed, c.info["largest_label"])
    if kind == "select_knn":
        radius, k, stat, lo, hi = e[1:6]
        found, _, d2 = kr.lists(pos, radius, k, mask)
        return kr.select(kr.values(found, d2, k, stat, mask), lo, np.inf if hi is None else hi, mask)
    raise AssertionError(e)


def merge_of(st, S, H, e):
    """merge_reference.merge of a ("merge_cells", cell, scope) entry on the scene `st`: the dict of the scene that is left"""
    n = st.n
    return _analysis_refs()[3].merge(st.data[:8 * n], st.positions[:3 * n], st.rotations[:4 * n], st.scales[:3 * n], e[1], scope_mask(e[2], S, H), H)


def _apply_edit(oracle, st, S, H, e):
    """one entry of State.edits on (SceneState, selection bool[n], hidden bool[n]); returns the new (S, H)"""
    er, ar, hr, sr, at = _refs()
    kind = e[0]
    if kind == "invert_selection":
        return ~S, H
    if kind in SELECT_KINDS or kind in ANALYSIS_PICKERS:
        return sr.apply_op(S, picked_by(oracle, st, S, H, e), e[-2] if kind == "select_region" else e[-1]), H
    if kind == "merge_cells":
        out = merge_of(st, S, H, e)
        if not out["info"]["merged_cells"]:      # nothing to merge: nothing changes, the selection included
            return S, H
        for name in ("data", "positions", "rotations", "scales"):
            setattr(st, name, np.ascontiguousarray(out[name]).reshape(-1))
        st.n = int(out["keep"].sum())
        return out["merged"].copy(), out["hidden"].copy()       # the selection becomes exactly the merged rows; H is carried
    if kind == "hide":
        return S, hr.hide_selected(H, S, e[1])
    if kind == "set_hidden":
        return S, hr.hidden_set(H, spec_set(e[1], st.n) if e[1] is not None else None, e[2])
    if kind == "edit":
        what, args, pivot = e[1], e[2], e[3]
        if what == "rgba":
            er.paint(st, S, args[0], args[1])
        else:
            er.apply(st, S, what, np.asarray(args, dtype=np.float64), pivot)
        return S, H
    if kind == "duplicate":
        if not S.any():                 # nothing selected: nothing touched, the selection included
            return S, H
        first, count = ar.duplicate(st, S)
        return ar.selection_after(st.n, first, count), ar.hidden_after(H, count)
    if kind == "append_arrays":
        add = oracle.SceneState(recipe_rows(("synth", e[1], e[2], "rows")))
        first, count = ar.append_arrays(st, add.data, add.positions, add.rotations, add.scales)
        return ar.selection_after(st.n, first, count), ar.hidden_after(H, count)
    if kind == "erase":
        gone = ~S if e[1] else S
        if not gone.any():              # nothing would be removed: nothing changes
            return S, H
        ar.erase(st, gone)
        return np.zeros(st.n, dtype=bool), hr.compact(H, ~gone)
    if kind == "transform":
        name, values = e[1], e[2]
        if name == "limit_box":
            keep = sr.box_pick(st.positions, values)
            st.limit_box(values)
            assert st.n == int(keep.sum())
            return np.zeros(st.n, dtype=bool), hr.compact(H, keep)
        getattr(st, name)(values)
        return S, H
    raise AssertionError(e)


def _evaluate(state, oracle):
    """(SceneState, S, H) of the State's recipe; memoised on the recipe's prefixes (the caller copies before it changes anything)"""
    import copy
    base = (state.scene, state.transforms)
    k = len(state.edits)
    while k > 0 and base + (state.edits[:k],) not in _mat_cache:
        k -= 1
    if base + (state.edits[:k],) in _mat_cache:
        st, S, H = _mat_cache[base + (state.edits[:k],)]
        st = copy.deepcopy(st)
    else:
        st = oracle.SceneState(recipe_rows(state.scene))
        for name, values in state.transforms:
            getattr(st, name)(values)
        S, H = np.zeros(st.n, dtype=bool), np.zeros(st.n, dtype=bool)
    for j in range(k, len(state.edits)):
        S, H = _apply_edit(oracle, st, S, H, state.edits[j])
        assert S.size == st.n and H.size == st.n
    key = base + (state.edits,)
    if key not in _mat_cache:
        if len(_mat_cache) >= _MAT_CACHE_MAX:
            _mat_cache.pop(next(iter(_mat_cache)))
        _mat_cache[key] = (copy.deepcopy(st), S.copy(), H.copy())
    return st, S, H


def materialise(state, oracle):
    """The scene, the selection and the hidden set the State's recipe leaves, evaluated on the CPU only: oracle.SceneState(rows),
    state.transforms with the oracle, state.edits with edit_reference, append_reference, hide_reference, select_reference,
    attr_reference and, for the analysis layer, neighbour_reference, cluster_reference, knn_reference and merge_reference (a merge
    hands over the merged arrays, the merged rows as the selection and the carried hidden set).  Arrays hold exactly n rows."""
    st, S, H = _evaluate(state, oracle)
    sr = _refs()[3]
    return Materialised(st.data[:8 * st.n].copy(), st.positions[:3 * st.n].copy(), st.rotations[:4 * st.n].copy(),
                        st.scales[:3 * st.n].copy(), st.n, sr.pack(S), sr.pack(H))


def vacuous(state, op, oracle):
    """Why `op`, performed from `state`, would check nothing (None: it checks something).  The conditions of the issue: a hide hides
    a listed splat and leaves one listed; a region or box selection picks more than none and fewer than all listed; an erase removes
    more than 0 and fewer than n; a contribution pass lists a selected and an unselected splat; nothing grows beyond MAX_GROWN.
    ANALYSIS_KINDS: _vacuous_analysis."""
    kind = op[0]
    if kind in ANALYSIS_KINDS:
        return _vacuous_analysis(state, op, oracle)
    if kind not in ("hide", "set_hidden", "select_box", "select_region", "erase", "contrib_pass", "duplicate", "append_arrays", "edit"):
        return None
    st, S, H = _evaluate(state, oracle)
    data = st.data[:8 * st.n]
    if kind == "edit":
        return None if S.any() else "nothing selected"
    if kind in ("hide", "set_hidden"):
        if "hide:on" not in tags(op, state):
            return None
        _, H1 = _apply_edit(oracle, st, S, H, op)
        before, after = listed_in(oracle, data, frame_of(state), H), listed_in(oracle, data, frame_of(state), H1)
        if not (before & H1 & ~H).any():
            return "hides no listed splat"
        return None if after.any() else "leaves nothing listed"
    if kind in ("select_box", "select_region"):
        e = fold(state, op).edits[-1]
        P = picked_by(oracle, st, S, H, e)
        L = listed_in(oracle, data, frame_of(state), H)
        if not P.any():
            return "picks nothing"
        return None if (L & ~P).any() else "picks every listed splat"
    if kind == "erase":
        gone = int((~S if op[1] else S).sum())
        return None if 0 < gone < st.n else "removes %d of %d" % (gone, st.n)
    if kind == "contrib_pass":
        L = listed_in(oracle, data, frame_of(state), H)
        return None if (L & S).any() and (L & ~S).any() else "lists no selected or no unselected splat"
    grown = st.n + (int(S.sum()) if kind == "duplicate" else op[1])
    if kind == "duplicate" and not S.any():
        return "nothing selected"
    return None if grown <= MAX_GROWN else "grows to %d" % grown


def _vacuous_analysis(state, op, oracle):
    """`vacuous` for ANALYSIS_KINDS.  A picker with "replace" picks a listed splat and leaves a listed one unpicked; an index seed of
    select_cluster_at is in scope and not noise; a merge merges a cell with a listed member, leaves a candidate unmerged and
    2 <= rows_after < n, and under scope "visible" a hidden splat sits in a cell that would merge without that scope; a merge and the
    cells report need a scene built from rows, a merge one without SH; nothing is analysed above MAX_ANALYSED splats."""
    kind = op[0]
    st, S, H = _evaluate(state, oracle)
    if st.n > MAX_ANALYSED:
        return "too large for the CPU fold"
    needs_rows = kind == "merge_cells" or (kind == "report" and op[1] == "cells")
    if needs_rows and st.n and scene_form(state.scene) != "rows":
        return "needs a scene built from rows"
    if kind == "report":
        return None
    nr, cr, kr, mr = _analysis_refs()
    n = st.n
    L = listed_in(oracle, st.data[:8 * n], frame_of(state), H) if n else np.zeros(0, dtype=bool)
    if kind in ANALYSIS_PICKERS:
        mask = scope_mask(op[-2], S, H)
        if kind == "select_cluster_at" and op[2] != "largest":
            if not (0 <= op[2] < n and mask[op[2]]):
                return "the seed is out of scope"
            if int(cr.Clusters(st.positions[:3 * n], op[1], op[3], mask).labels[op[2]]) == cr.NONE:
                return "the seed is noise"
        if op[-1] != "replace":
            return None
        P = analysis_pick(st, mask, op)
        if not (L & P).any():
            return "picks no listed splat"
        return None if (L & ~P).any() else "picks every listed splat"
    if state.sh is not None:
        return "SH rows present"
    cell, scope = op[1], op[2]
    arrays = (st.positions[:3 * n], st.rotations[:4 * n], st.scales[:3 * n])
    cand, _, members = mr.cells_of(*arrays, cell, scope_mask(scope, S, H))
    merging = [i for idx in members.values() if len(idx) >= 2 for i in idx]
    if not L[merging].any():
        return "merges no cell with a listed member"
    if len(merging) >= int(cand.sum()):
        return "leaves no candidate unmerged"
    rows_after = n - len(merging) + sum(len(idx) >= 2 for idx in members.values())
    if not 2 <= rows_after < n:
        return "leaves %d of %d rows" % (rows_after, n)
    if "visible" in scope:      # a hidden splat in a cell that would otherwise merge: the scope keeps something out
        _, _, wider = mr.cells_of(*arrays, cell, scope_mask(tuple(x for x in scope if x != "visible"), S, H))
        if not any(len(idx) >= 2 and H[idx].any() for idx in wider.values()):
            return "no hidden splat in a cell that would otherwise merge"
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# Traces
# ---------------------------------------------------------------------------------------------------------------------------
def _band_for(W):
    x0 = (W // 3) // 32 * 32
    return (x0, min(W, x0 + max(32, (W // 4) // 32 * 32 + 17)))     # (x1 off a bin boundary: the last bin column is partial)


BOX = (-1.25, 1.5, -2.0, 1.0, -1.5, 1.25)
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)


def tour(band_context=False):
    """The fixed trace: every operation, every read-back and refusal, every pair of RISKY_PAIRS, sizes on both sides of the 4096-bin
    boundary (two-level binning above it, two compositor waves per tile up to it) and scene sizes 0 .. 3.2 M (both keys-per-block
    steps and the bucket order's limit).  band_context: the trace of a context created with a band -- gsr_resize drops the band,
    so every resize is followed by a gsr_set_band for the new width."""
    C, N = True, False
    t = []

    def add(*op, check=C):
        t.append(Step(tuple(op), check))

    def size(W, H):
        add("resize", W, H)
        if band_context:
            add("band", *_band_for(W))

    # cameras, read-backs, sort-only frames on the first scene (contexts with stage events: every other frame carries them, the
    # others are graph replays)
    add("timing_interval", 2)
    add("camera", 7)
    add("same_pose")
    add("burst", 8, 9, 10, check=N)
    add("readback", "keys")
    add("readback", "records", check=N)
    add("camera", 11)                                   # records -> the next frame (individual launches or a first capture)
    add("readback", "records", check=N)
    add("same_pose")                                    # records -> graph replay
    for which in ("bin_lists", "work_items", "depth_index", "read_depth", "pick", "stats"):
        add("readback", which, check=N)
    add("sort_only", 1, 30, check=N)
    add("readback", "records")
    add("sort_only", 2, 31, check=N)
    add("readback", "depth_index")
    # band on, moved, off, on again with the earlier band
    add("band", 192, 448)
    add("readback", "records", check=N)
    add("camera", 12)
    add("band", 320, 600)
    add("band", 96, 300)
    add("band", 0, 0)
    add("band", 192, 448)
    add("sort_only", 1, 33)
    add("band", 0, 0)
    if band_context:
        add("band", 192, 448)
    # scenes of other sizes, growing and shrinking, rows and raw
    add("scene", ("synth", 0, 1, "raw"))
    add("sort_only", 2, 34, check=N)
    add("scene", ("synth", 1, 2, "rows"))
    add("scene", ("synth", 63, 3, "raw"))
    add("scene", ("synth", 70000, 4, "rows"))
    add("camera", 13)
    add("scene", ("synth", 2049, 5, "raw"))
    add("camera", 14)
    add("scene", ("synth", 300000, 6, "raw"))
    add("camera", 15)
    add("scene", ("synth", 3200000, 8, "rows"))          # above 3 << 20: 4096 keys per block, the LSD order only
    add("camera", 16)
    add("scene", ("config", "C1", "rows"))
    add("camera", 17)
    # transforms, SH, limit box
    add("rotate", QUAT)
    add("translate", (0.25, -0.125, 0.5))
    add("scale", (1.25, 0.75, 1.0))
    add("sh", (11, 0.0, 0.25, 0.5))
    add("camera", 18)
    add("sh", (12, 0.5, 0.5, 0.75))
    add("sh", None)
    add("sh", (11, 0.0, 0.25, 0.5))
    add("limit_box", BOX)
    add("sh", (13, 0.0, 0.5, 0.5))
    add("camera", 19)
    # depth fade, hit alpha, depth planes
    add("fade", True, 0.3)
    add("fade", False, 0.0)
    add("fade", True, 0.8)
    add("hit_alpha", 0.9)
    add("depth_async", False)
    add("camera", 20)
    add("depth_async", True)
    add("hit_alpha", 0.25)
    add("fade", False, 0.0)
    # stage events and graph replays, alternating
    add("timing_interval", 2)
    add("camera", 21)
    add("same_pose")
    add("timing_interval", 0xffffffff)
    add("camera", 22)
    add("timing_interval", 1)
    add("camera", 23)
    # sizes: odd, across the 4096-bin boundary in both directions, a shrink followed by the original size
    add("sort_only", 1, 35, check=N)
    size(333, 219)
    add("band", 64, 200)
    size(640, 480)
    size(2048, 2048)                                     # 4096 bins: one-level binning, two waves per tile (default contexts)
    size(2080, 2048)                                     # 4160 bins: two-level, one wave per tile
    add("camera", 24)
    size(2048, 2048)
    size(3840, 2160)
    add("band", 1728, 2208)                              # a band on a 4K frame: survivor sort and gather
    add("camera", 25)
    add("band", 0, 0)
    if band_context:
        add("band", 1728, 2208)
    size(1279, 717)
    size(640, 480)
    # list overflow: repaired by sync; three frames queued behind it
    add("scene", ("synth", 70000, 4, "raw"))
    add("overflow_sync", 2048)
    add("scene", ("synth", 20000, 9, "rows"))
    add("overflow_async", 2048, 40, 41, 42)
    add("band", 192, 448)
    add("overflow_async", 1024, 43, 44, 45)
    add("scene", ("synth", 70000, 4, "rows"))
    add("band", 0, 0)
    if band_context:
        add("band", 192, 448)
    # delivery rings
    add("ring_open", "rgba8", False, None, 1)
    add("deliver")
    add("resize", 801, 601)
    add("deliver")
    if band_context:
        add("band", *_band_for(801))
    add("ring_close")
    add("ring_open", "nv12", False, None, 1)
    add("deliver", check=N)
    add("camera", 26)
    add("ring_close")
    add("ring_open", "i420", True, "u16", 2)
    size(640, 480)
    add("deliver")
    add("ring_close")
    add("ring_open", "rgba8", False, "f32", 1)
    add("camera", 27)
    add("ring_close")
    add("ring_open", "nv12", True, "u16", 1)
    add("camera", 28)
    add("ring_close")
    add("ring_open", "rgba8", False, "f32", 2)
    add("camera", 29)
    add("ring_close")
    # refused calls
    add("sh", (14, 0.0, 0.25, 0.5))
    for which in REFUSALS:
        add("refused", which)
        add("camera", 50 + REFUSALS.index(which))
    return t


SELOPS = ("replace", "add", "subtract", "intersect")
ALL = (1, 2.0)                          # a set_selection / set_hidden spec that names every splat
RECT = (224, 120, 416, 360)             # inside the band (192, 448) of a 640 x 480 frame
DISC = ("disc", 320.5, 240.5, 90.0, 5)  # select_reference.disc: rows 5 bytes longer than the rectangle, the padding non-zero
PIVOT = (0.25, -0.5, 0.125)
OUTLINE_OUTER = ((1.0, 1.0, 1.0), 1.0, 0.5, 2, "outer")
OUTLINE_INNER = ((0.0, 1.0, 0.25), 0.75, 0.25, 5, "inner")


def editing_tour(band_context=False):
    """The fixed trace of the editing layer: every kind of EDIT_KINDS, every refusal of EDIT_REFUSALS, every pair of EDIT_RISKY_PAIRS,
    on small scenes (1, 33, 2049 and 20 000 splats built from rows, growing to at most MAX_GROWN) and small frames (at most
    900 x 700, and one size above 4096 bins for two-level binning).  It starts from State()'s raw scene, where hiding and selecting
    work and editing is refused.  band_context: as in tour()."""
    C, N = True, False
    t = []

    def add(*op, check=C):
        t.append(Step(tuple(op), check))

    def size(W, H):
        add("resize", W, H)
        if band_context:
            add("band", *_band_for(W))

    def band_off():
        add("band", 0, 0)
        if band_context:
            add("band", 192, 448)

    def box(f):
        return tuple(v * f for v in BOX)

    # a raw scene: pickers and hides work, edits and erases are refused
    add("set_selection", (3, 0.5), "replace", check=N)
    add("refused", "edit_raw")
    add("camera", 60)
    add("refused", "erase_raw")
    add("camera", 61)
    add("hide", "add")
    add("same_pose")                                    # the graph captured without a mask is not replayed
    add("set_hidden", (5, 0.4), "replace")
    add("set_hidden", None, "replace")                  # show all: the null pointer again, the buffers stay
    add("same_pose")
    add("hide", "add")
    add("band", 192, 448)
    add("set_hidden", (6, 0.5), "add")
    add("overflow_sync", 2048)
    add("set_hidden", (7, 0.3), "add")
    add("overflow_async", 1024, 40, 41, 42)
    add("set_hidden", (8, 0.2), "add")
    add("sort_only", 1, 30)
    add("readback", "records", check=N)
    add("hide", "subtract")                             # show the selected ones
    band_off()
    add("set_hidden", (9, 0.5), "replace")
    add("scene", ("synth", 33, 2, "rows"))              # nothing hidden again
    add("set_hidden", (10, 0.5), "replace")
    add("select_hidden", "replace", check=N)
    add("edit", "translate", (0.25, 0.0, -0.125), None)
    # one splat
    add("scene", ("synth", 1, 3, "rows"))
    add("set_selection", ALL, "replace", check=N)
    add("edit", "scale", (1.5, 1.0, 0.5), None)
    add("duplicate", "grow")
    add("edit", "translate", (0.0, 0.25, 0.0), None)
    # edits of the selection
    add("scene", ("synth", 2049, 5, "rows"))
    add("select_box", box(0.5), "replace", check=N)
    add("edit", "translate", (0.5, -0.25, 0.125), None)
    add("same_pose")
    add("edit", "rotate", QUAT, None)
    add("sort_only", 1, 31)
    add("edit", "rotate", QUAT, PIVOT)
    add("readback", "pick", check=N)
    add("camera", 62)
    add("edit", "scale", (1.25, 0.75, 1.0), None)
    add("edit", "scale", (0.5, 1.0, 2.0), PIVOT)
    add("edit", "rgba", (0x00c08040, 0x00ffffff), None)
    add("edit", "rgba", (0x60000000, 0xff000000), None)
    # pickers: a rectangle and a byte mask, all four fold ops
    add("select_region", RECT, None, "replace", check=N)
    add("camera", 63)
    add("select_region", disc_rect(DISC), DISC, "add")
    add("select_region", (256, 200, 352, 300), None, "subtract", check=N)
    add("select_region", disc_rect(DISC), DISC, "intersect")
    add("invert_selection")
    add("select_attr", "opacity", 0.0, 128.0, None, "replace", check=N)
    add("select_attr", "distance", 0.0, 1.5, (0.5, 0.0, -0.25), "add")
    add("select_attr", "scale_max", 0.0, 0.05, None, "subtract")
    add("set_hidden", (11, 0.3), "replace")
    add("select_hidden", "add", check=N)
    add("select_box", box(1.0), "intersect")
    add("limit_box", BOX)                               # the selection does not survive, the hidden set is carried
    add("select_box", box(0.5), "replace", check=N)
    add("hide", "add")
    add("limit_box", box(0.75))
    add("set_selection", (16, 0.3), "replace", check=N)
    add("hide", "replace")
    add("erase", False)                                 # the hidden selected splats go; H is carried
    add("set_selection", (12, 0.5), "replace", check=N)
    add("erase", True)
    add("select_box", box(0.3), "replace")
    add("scene", ("synth", 2049, 5, "rows"))
    # growth: beyond the capacity, inside it, inside a reserve
    add("set_selection", ALL, "replace", check=N)
    add("duplicate", "grow")                            # 2049 -> 4098: past sort.rows and past two blocks of 2048 keys
    add("sort_only", 1, 32)
    add("set_selection", (2, 0.1), "replace", check=N)
    add("duplicate", "grow")                            # capacity 4098 -> 6147
    add("same_pose")
    add("set_selection", (3, 0.1), "replace", check=N)
    add("duplicate", "fit")
    add("same_pose")
    add("reserve", 20000)
    add("same_pose")
    add("duplicate", "fit")
    add("burst", 64, 65, 66)
    add("edit", "translate", (0.0, 0.5, 0.0), None)     # the copies move
    add("duplicate", "fit")
    add("band", 192, 448)
    band_off()
    add("duplicate", "fit")
    size(333, 219)
    size(640, 480)
    add("duplicate", "fit")
    add("erase", False)                                 # the copies go again
    add("set_selection", (4, 0.05), "replace", check=N)
    add("duplicate", "fit")                             # onto the rows the compaction left stale
    add("append_arrays", 500, 21)
    add("limit_box", BOX)
    add("append_arrays", 33, 22)
    add("invert_selection")
    add("erase", True)                                  # only the appended rows' complement stays selected: keep it
    add("band", 192, 448)
    band_off()
    # the overlay
    add("scene", ("synth", 20000, 9, "rows"))
    add("select_box", box(0.5), "replace", check=N)
    add("overlay", (1.0, 0.5, 0.0), 0.5, None, check=N)
    add("resize", 801, 601)
    if band_context:
        add("band", *_band_for(801))
    size(640, 480)
    add("overlay", (0.0, 0.5, 1.0), 0.75, OUTLINE_OUTER)
    add("set_hidden", (13, 0.4), "add")
    add("overlay", (0.0, 0.5, 1.0), 0.75, None)
    add("duplicate", "grow")
    add("overlay", (1.0, 0.0, 0.0), 1.0, OUTLINE_INNER)
    add("band", 192, 448)
    band_off()
    add("ring_open", "rgba8", False, None, 1)
    add("ring_overlay", True)
    add("deliver")
    add("ring_overlay", True)
    add("resize", 512, 384)
    add("deliver")
    if band_context:
        add("band", *_band_for(512))
    add("ring_close")
    add("ring_open", "nv12", False, "u16", 2)
    add("ring_overlay", True)
    size(640, 480)
    add("deliver")
    add("ring_overlay", True)
    add("overlay", None)                                # off under a ring that delivers it: deliveries are refused, no slot is taken
    add("deliver")
    add("overlay", (1.0, 0.5, 0.0), 0.5, None)          # options again: the ring's switch stayed, it delivers the overlay again
    add("deliver", check=N)
    add("ring_overlay", True)
    add("ring_overlay", False)
    add("overlay", None)
    add("ring_close")
    # two-level binning (above 4096 bins) with a hidden set and a grown scene
    size(2080, 2048)
    add("set_hidden", (14, 0.5), "replace")
    add("select_box", box(0.3), "replace", check=N)
    add("duplicate", "fit")
    size(640, 480)
    # contribution
    add("scene", ("synth", 2049, 5, "rows"))
    add("select_box", box(0.5), "replace", check=N)
    add("contrib_reset")
    add("contrib_pass", check=N)
    add("camera", 67)
    add("contrib_pass")
    add("select_contrib", "weight", np.inf, "intersect", check=N)
    add("contrib_pass", check=N)
    add("duplicate", "grow")                            # the accumulators grow with zeros
    add("contrib_pass", check=N)
    add("erase", False)                                 # ... and are dropped
    add("select_box", box(0.5), "replace", check=N)
    add("contrib_pass")                                 # never reset: the first pass resets first
    add("select_contrib", "pixels", 0.0, "subtract")
    add("contrib_pass", check=N)
    add("scene", ("synth", 2049, 6, "rows"))
    # refusals that need SH rows, and an upload that contradicts itself
    add("set_selection", (15, 0.5), "replace", check=N)
    add("sh", (11, 0.0, 0.25, 0.5))
    add("refused", "grow_with_sh")
    add("camera", 68)
    add("refused", "rotate_selected_sh_follow")
    add("camera", 69)
    add("sh", None)
    add("refused", "append_positions_differ")
    add("camera", 70)
    return t


def analysis_spacing(n):
    """The radius at which a splat in the middle of a synth scene of n splats has about three neighbours.  The scenes of every trace
    are gsplat_hip.synth's: positions drawn from a gaussian of standard deviation 1.5 per axis, so the density in the middle is
    n / ((2 pi)^1.5 * 1.5^3) = n / 53.2 per unit volume, and 4/3 pi r^3 of it holds three at r = 3.4 * n^(-1/3) (0.27 at 2049 splats).
    Radii and cell sides of the traces and of the observables are small multiples of it."""
    return 3.4 * max(int(n), 1) ** (-1.0 / 3.0)


COINCIDENT = 2.0 ** -10     # a cell side at which, in these scenes, little but a copy and its original share a cell
CLUSTER_SEED = 0            # an index that is labelled where analysis_tour seeds select_cluster_at (tests/test_history_trace.py asks `vacuous`)


def analysis_tour(band_context=False):
    """The fixed trace of the analysis layer: every kind of ANALYSIS_KINDS with every scope and every fold op, every refusal of
    ANALYSIS_REFUSALS, every pair of ANALYSIS_RISKY_PAIRS, on rows scenes of 2049, 4099, 2601 and 6001 splats (more than one
    workgroup of 256 and a partial last wave each; merges shrink them, duplicates grow them past the scratch of the scene before) at
    640 x 480 and one other size.  It starts from State()'s raw scene, where the pickers work and a merge is refused.  Every radius
    differs from the one of the call before.  band_context: as in tour()."""
    C, N = True, False
    t = []
    h = analysis_spacing(2049)

    def add(*op, check=C):
        t.append(Step(tuple(op), check))

    def size(W, H):
        add("resize", W, H)
        if band_context:
            add("band", *_band_for(W))

    def band_off():
        add("band", 0, 0)
        if band_context:
            add("band", 192, 448)

    sel, vis, both = ("selected",), ("visible",), ("selected", "visible")
    # a raw scene: the pickers and three of the reports work on positions alone, a merge is refused
    add("refused", "merge_raw")
    add("camera", 60)
    add("select_neighbours", 1.1 * h, 1, None, 8, (), "replace")
    add("report", "knn", 1.3 * h, 4, "kth", (), check=N)
    add("same_pose")
    # different features back to back over the one index, a different radius each time
    add("scene", ("synth", 2049, 5, "rows"))
    add("select_neighbours", 1.2 * h, 1, None, 16, (), "replace", check=N)
    add("select_knn", 1.6 * h, 4, "mean", 0.0, 1.2 * h, (), "add")
    add("select_clusters", 0.9 * h, 2, None, 0, (), "intersect")
    add("merge_cells", 0.5 * h, ())
    add("select_neighbours", 1.4 * h, 0, 1, 8, (), "replace")          # the floaters of the merged scene
    add("merge_cells", 0.7 * h, ())
    add("merge_cells", 0.9 * h, ())                                     # a larger cell over the rows the merge before wrote
    add("same_pose")
    # the statistical outlier filter: the threshold is a constant of the trace
    add("select_knn", 2.0 * h, 8, "mean", 1.5 * h, None, (), "replace")
    add("erase", False)
    add("select_cluster_at", 1.5 * h, "largest", 0, (), "replace")
    add("select_cluster_at", 1.25 * h, CLUSTER_SEED, 1, (), "add")
    add("select_clusters", 1.0 * h, 0, 3, 2, (), "subtract")
    # merge and the hidden set, in both scopes; scopes of the pickers
    add("scene", ("synth", 2049, 5, "rows"))
    add("set_hidden", (21, 0.3), "replace")
    add("merge_cells", 0.6 * h, ())                                     # hidden members merge, H is carried with the leaders
    add("sort_only", 1, 30)
    add("set_hidden", (22, 0.3), "add")
    add("select_neighbours", 1.3 * h, 1, None, 4, vis, "replace")
    add("merge_cells", 0.8 * h, vis)                                    # a hidden member stays out of its cell
    add("set_hidden", None, "replace")                                  # show all
    add("set_selection", (23, 0.6), "replace", check=N)
    add("select_knn", 1.7 * h, 2, "kth", 0.0, 1.1 * h, sel, "intersect")
    add("select_clusters", 1.2 * h, 2, None, 1, sel, "replace")
    add("set_selection", (24, 0.7), "replace", check=N)
    add("merge_cells", 1.0 * h, sel)
    add("burst", 64, 65, 66)
    add("set_hidden", (25, 0.25), "replace")
    add("set_selection", (26, 0.7), "replace", check=N)
    add("select_cluster_at", 1.6 * h, "largest", 0, both, "intersect")
    add("select_knn", 1.4 * h, 3, "mean", 0.0, 1.0 * h, both, "add")
    add("select_neighbours", 1.9 * h, 2, 5, 4, both, "subtract")
    add("select_clusters", 1.3 * h, 0, 2, 0, vis, "add")
    add("set_selection", (27, 0.7), "replace", check=N)
    add("merge_cells", 1.2 * h, both)
    add("readback", "records", check=N)
    add("camera", 61)
    add("set_hidden", None, "replace")
    # reports disturb neither frame nor scene
    for which, args in (("neighbours", (1.1 * h, 16, ())), ("clusters", (1.4 * h, 2, vis)), ("knn", (1.7 * h, 8, "mean", sel)), ("cells", (0.9 * h, 8, both))):
        add("report", which, *args, check=N)
        add("same_pose")
        add("report", which, *args, check=N)
        add("readback", "bin_lists", check=N)
    # the same radius twice in a row under another scope: an index kept for its radius alone would hold the wrong splats
    add("set_selection", (29, 0.5), "replace", check=N)
    add("report", "neighbours", 1.2 * h, 8, (), check=N)
    add("select_neighbours", 1.2 * h, 1, None, 8, sel, "replace")
    # scratch sizing: a larger scene, a smaller one, a report in front of the edit
    add("scene", ("synth", 4099, 7, "rows"))
    add("merge_cells", 0.6 * h, ())                                     # both shares of the merge scratch grow
    add("band", 192, 448)
    add("merge_cells", 0.8 * h, ())                                     # behind a band frame
    add("band", 320, 600)
    band_off()
    add("merge_cells", 1.0 * h, ())
    size(333, 219)
    size(640, 480)
    add("scene", ("synth", 2601, 8, "rows"))
    add("merge_cells", 0.5 * h, ())                                     # scratch larger than the scene
    # capacity above n: the copies merge with their originals
    add("set_selection", (28, 0.65), "replace", check=N)
    add("duplicate", "grow")                                            # past the 4099 rows the scratch was sized for
    add("merge_cells", COINCIDENT, ())
    add("duplicate", "fit")                                             # the merged rows again, onto the rows the compaction left stale
    add("merge_cells", COINCIDENT, ())
    add("reserve", 9000)
    add("merge_cells", 0.7 * h, ())
    add("append_arrays", 500, 21)
    add("merge_cells", 0.9 * h, ())
    add("erase", False)                                                 # the merged rows go
    add("select_cluster_at", 1.5 * h, CLUSTER_SEED, 0, (), "replace")
    add("scene", ("synth", 6001, 9, "rows"))
    add("report", "cells", 0.4 * h, 4, (), check=N)                     # the report's share of the scratch only
    add("merge_cells", 0.4 * h, ())
    # frames in flight and regrown lists in front of the merge
    add("burst", 67, 68, 69, check=N)
    add("merge_cells", 0.5 * h, ())
    add("overflow_async", 1024, 40, 41, 42)
    add("merge_cells", 0.6 * h, ())
    # pickers behind a change of positions, numbering or hidden set
    add("scene", ("synth", 2049, 5, "rows"))
    add("select_box", tuple(v * 0.5 for v in BOX), "replace", check=N)
    add("edit", "translate", (0.5, -0.25, 0.125), None)
    add("select_neighbours", 1.2 * h, 1, None, 8, (), "replace")
    add("translate", (0.25, -0.125, 0.5))
    add("select_knn", 1.5 * h, 4, "kth", 0.0, 1.25 * h, (), "replace")
    add("limit_box", BOX)
    add("select_clusters", 1.1 * h, 2, None, 0, (), "replace")
    add("hide", "add")
    add("select_neighbours", 1.3 * h, 0, 1, 8, vis, "replace")
    add("set_hidden", None, "replace")
    # the layers that follow the selection
    add("select_box", tuple(v * 0.5 for v in BOX), "replace", check=N)
    add("contrib_reset")
    add("contrib_pass", check=N)
    add("merge_cells", 0.5 * h, ())                                     # the accumulators are dropped
    add("overlay", (1.0, 0.5, 0.0), 0.5, OUTLINE_OUTER, check=N)
    add("merge_cells", 0.7 * h, ())                                     # the overlay tints the merged rows
    add("ring_open", "rgba8", False, None, 1)
    add("ring_overlay", True)
    add("merge_cells", 0.9 * h, ())
    add("deliver")
    add("ring_overlay", False)
    add("overlay", None)
    add("ring_close")
    # refusals
    for which in ANALYSIS_REFUSALS:
        if which == "merge_raw":
            continue                                                    # (at the head of the trace, on the raw scene)
        if which == "merge_with_sh":
            add("sh", (11, 0.0, 0.25, 0.5))
        add("refused", which)
        add("camera", 70 + ANALYSIS_REFUSALS.index(which))
    return t


WALK_SIZES = ((640, 480), (333, 219), (900, 700), (64, 64), (801, 601), (512, 384), (160, 96))
WALK_SCENES = (0, 1, 63, 2049, 20000, 7000, 300, 12000)
WALK_RINGS = (("rgba8", False, None, 1), ("nv12", False, None, 1), ("i420", True, None, 1), ("rgba8", False, "u16", 1),
              ("nv12", True, "f32", 2), ("i420", False, "u16", 2), ("rgba8", False, "f32", 1))


def _gen(kind, s, rng):
    """operations that perform one `kind` from State `s` (a prelude where the kind needs one: rows for a transform, a ring for a delivery)"""
    pose = rng.randrange(120)
    rows_scene = ("scene", ("synth", rng.choice((2049, 7000, 20000)), rng.randrange(1, 50), "rows"))
    need_rows = [] if scene_form(s.scene) == "rows" else [rows_scene]
    if kind == "camera":
        return [("camera", pose)]
    if kind == "same_pose":
        return [("same_pose",)]
    if kind == "burst":
        return [("burst", pose, (pose + 1) % 120, (pose + 2) % 120)]
    if kind == "sort_only":
        return [("sort_only", rng.choice((1, 2)), pose)]
    if kind == "readback":
        return [("readback", rng.choice(READBACKS))]
    if kind == "scene":
        return [("scene", ("synth", rng.choice(WALK_SCENES), rng.randrange(1, 50), rng.choice(("rows", "raw"))))]
    if kind == "resize":
        return [("resize",) + rng.choice([z for z in WALK_SIZES if z != (s.W, s.H)])]
    if kind == "band":
        if s.band is not None and rng.random() < 0.4:
            return [("band", 0, 0)]
        x0 = rng.randrange(0, max(1, (s.W - 1) // 32 + 1)) * 32
        return [("band", x0, x0 + rng.choice((32, 64, 100, 257, 10000)))]
    if kind == "sh":
        if s.sh is not None and rng.random() < 0.4:
            return [("sh", None)]
        f = sorted(rng.choice((0.0, 0.25, 0.5, 0.75)) for _ in range(3))
        return [("sh", (rng.randrange(1, 99), f[0], f[1], f[2]))]
    if kind == "limit_box":
        return need_rows + [("limit_box", tuple(v * rng.choice((0.75, 1.0, 1.5)) for v in BOX))]
    if kind == "rotate":
        q = [rng.uniform(-1, 1) for _ in range(4)]
        ln = sum(v * v for v in q) ** 0.5 or 1.0
        return need_rows + [("rotate", tuple(v / ln for v in q))]
    if kind == "translate":
        return need_rows + [("translate", tuple(rng.choice((-0.5, -0.125, 0.0, 0.25, 0.5)) for _ in range(3)))]
    if kind == "scale":
        return need_rows + [("scale", tuple(rng.choice((0.75, 1.0, 1.25)) for _ in range(3)))]
    if kind == "fade":
        return [("fade", False, 0.0)] if s.fade[0] and rng.random() < 0.5 else [("fade", True, rng.choice((0.2, 0.5, 0.8)))]
    if kind == "hit_alpha":
        return [("hit_alpha", rng.choice([a for a in (0.1, 0.25, 0.5, 0.9, 1.0) if a != s.hit_alpha]))]
    if kind == "depth_async":
        return [("depth_async", rng.random() < 0.5)]
    if kind == "timing_interval":
        return [("timing_interval", rng.choice((1, 2, 3, 0xffffffff)))]
    if kind == "overflow_sync":
        return [("overflow_sync", rng.choice((1024, 2048)))]
    if kind == "overflow_async":
        return [("overflow_async", rng.choice((1024, 2048)), pose, (pose + 5) % 120, (pose + 10) % 120)]
    if kind == "ring_open":
        return ([("ring_close",)] if s.ring else []) + [("ring_open",) + rng.choice([g for g in WALK_RINGS if g != s.ring])]
    if kind == "ring_close":
        return ([] if s.ring else [("ring_open",) + rng.choice(WALK_RINGS)]) + [("ring_close",)]
    if kind == "deliver":
        return ([] if s.ring else [("ring_open",) + rng.choice(WALK_RINGS)]) + [("deliver",)]
    if kind == "refused":
        return [("refused", rng.choice(REFUSALS))]
    raise AssertionError(kind)


def _picker(s, rng):
    """one picker that needs nothing but a scene (a region picks from the frame of the State's pose)"""
    selop = rng.choice(SELOPS)
    kind = rng.choice(("select_box", "select_region", "select_region", "set_selection", "select_attr"))
    if kind == "select_box":
        f = rng.choice((0.3, 0.5, 0.75))
        return ("select_box", tuple(v * f for v in BOX), selop)
    if kind == "select_region":
        x0, x1 = s.band if s.band is not None else (0, s.W)
        w = x1 - x0
        if rng.random() < 0.5 and min(w, s.H) >= 12:
            mspec = ("disc", x0 + w / 2.0, s.H / 2.0, float(min(w, s.H) // 3), rng.choice((0, 3)))
            return ("select_region", disc_rect(mspec), mspec, selop)
        return ("select_region", (x0 + w // 4, s.H // 4, x0 + max(w // 4 + 1, 3 * w // 4), max(s.H // 4 + 1, 3 * s.H // 4)), None, selop)
    if kind == "set_selection":
        return ("set_selection", (rng.randrange(1, 99), rng.choice((0.1, 0.5))), selop)
    attr = rng.choice(("x", "opacity", "distance") + (("scale_max",) if scene_form(s.scene) == "rows" else ()))
    lo, hi, origin = {"x": (-0.5, 0.75, None), "opacity": (0.0, 128.0, None), "distance": (0.0, 1.5, (0.5, 0.0, -0.25)),
                      "scale_max": (0.0, 0.05, None)}[attr]
    return ("select_attr", attr, lo, hi, origin, selop)


def _gen_edit(kind, s, rng):
    """_gen for the kinds of EDIT_KINDS and ("refused_edit",): the operations, preludes included.  Which splats a step touches depends
    on the scene: walk() asks `vacuous` and draws again."""
    rows_scene = ("scene", ("synth", rng.choice((2049, 7000, 20000)), rng.randrange(1, 50), "rows"))
    small = scene_n(s.scene) < 33
    need_scene = [rows_scene] if small else []
    need_rows = [rows_scene] if small or scene_form(s.scene) != "rows" else []
    sh_now = None if need_rows else s.sh
    picker = [_picker(fold_ops(s, need_rows), rng)] if rng.random() < 0.5 else []
    no_sh = [("sh", None)] if sh_now is not None else []
    # (what a region picks and what a pass lists depends on the pose: some of the draws move the camera first)
    cam = [("camera", rng.randrange(120))] if rng.random() < 0.5 else []
    if kind in ("select_box", "select_region", "set_selection", "select_attr"):
        while True:
            op = _picker(fold_ops(s, need_scene), rng)
            if op[0] == kind:
                return need_scene + (cam if kind == "select_region" else []) + [op]
    if kind == "invert_selection":
        return need_scene + [("invert_selection",)]
    if kind == "select_hidden":
        return need_scene + [("select_hidden", rng.choice(SELOPS))]
    if kind == "select_contrib":
        pre = [] if s.contrib and not need_scene else cam + [("set_selection", (rng.randrange(1, 99), 0.5), "replace"), ("contrib_pass",)]
        return need_scene + pre + [("select_contrib", rng.choice(("weight", "peak", "pixels")), rng.choice((np.inf, 0.0)), rng.choice(SELOPS))]
    if kind == "hide":
        return need_scene + ([_picker(fold_ops(s, need_scene), rng)] if picker else []) + [("hide", rng.choice(SELOPS))]
    if kind == "set_hidden":
        if rng.random() < 0.25:
            return need_scene + [("set_hidden", None, "replace")]
        return need_scene + [("set_hidden", (rng.randrange(1, 99), rng.choice((0.2, 0.5))), rng.choice(SELOPS))]
    if kind == "edit":
        what = rng.choice(("translate", "rotate", "scale", "rgba"))
        pivot = None if what in ("translate", "rgba") or rng.random() < 0.5 else PIVOT
        args = {"translate": tuple(rng.choice((-0.5, -0.125, 0.0, 0.25)) for _ in range(3)), "rotate": QUAT,
                "scale": tuple(rng.choice((0.5, 1.0, 1.25)) for _ in range(3)),
                "rgba": (rng.randrange(1 << 32), rng.choice((0x00ffffff, 0xff000000, 0xffffffff, 0x0000ff00)))}[what]
        return need_rows + picker + [("edit", what, args, pivot)]
    if kind == "reserve":
        return need_rows + no_sh + [("reserve", rng.choice((1000, 25000, 30000, 40000)))]
    if kind == "duplicate":
        return need_rows + no_sh + picker + [("duplicate", None)]
    if kind == "append_arrays":
        return need_rows + no_sh + [("append_arrays", rng.choice((1, 33, 500)), rng.randrange(1, 50))]
    if kind == "erase":
        return need_rows + no_sh + picker + [("erase", rng.random() < 0.5)]
    if kind == "overlay":
        if s.overlay is not None and rng.random() < 0.3:
            return [("overlay", None)]
        tint = tuple(rng.choice((0.0, 0.5, 1.0)) for _ in range(3))
        return [("overlay", tint, rng.choice((0.25, 0.5, 1.0)), rng.choice((None, OUTLINE_OUTER, OUTLINE_INNER)))]
    if kind == "ring_overlay":
        if s.ring_overlay:
            return [("ring_overlay", False)]
        return (([] if s.ring else [("ring_open",) + rng.choice(WALK_RINGS)]) +
                ([] if s.overlay else [("overlay", (1.0, 0.5, 0.0), 0.5, OUTLINE_OUTER)]) + [("ring_overlay", True), ("deliver",)])
    if kind == "contrib_reset":
        return [("contrib_reset",)]
    if kind == "contrib_pass":
        half = [("set_selection", (rng.randrange(1, 99), 0.5), "replace")] if rng.random() < 0.6 else []
        return need_scene + cam + half + [("contrib_pass",)]
    if kind == "refused_edit":
        which = rng.choice(EDIT_REFUSALS)
        some = ("set_selection", (rng.randrange(1, 99), 0.5), "replace")
        if which in ("edit_raw", "erase_raw"):
            raw = [] if scene_form(s.scene) == "raw" and not small else [("scene", ("synth", rng.choice((2049, 7000)), rng.randrange(1, 50), "raw"))]
            return raw + [some, ("refused", which)]
        if which == "append_positions_differ":
            return need_rows + no_sh + [("refused", which)]
        return need_rows + ([] if sh_now is not None else [("sh", (rng.randrange(1, 99), 0.0, 0.25, 0.5))]) + [some, ("refused", which)]
    raise AssertionError(kind)


def _gen_analysis(kind, s, rng, oracle):
    """_gen for the kinds of ANALYSIS_KINDS and ("refused_analysis",).  The CPU fold of these is blocked brute force, so they are
    generated on rows scenes of 33 .. MAX_ANALYSED splats only: a scene that is raw, smaller or has grown beyond that is replaced first.
    Radii and cell sides are multiples of the scene's own spacing (analysis_spacing); what a step picks or merges depends on the
    scene: walk() asks `vacuous` and draws again."""
    rows_scene = ("scene", ("synth", rng.choice((2049, 3000, 4100)), rng.randrange(1, 50), "rows"))
    n_now = _evaluate(s, oracle)[0].n
    fits = scene_form(s.scene) == "rows" and 33 <= n_now <= MAX_ANALYSED
    pre = [] if fits else [rows_scene]
    n = n_now if fits else rows_scene[1][1]
    sh_now = s.sh if fits else None
    h = analysis_spacing(n)
    some = ("set_selection", (rng.randrange(1, 99), rng.choice((0.5, 0.7))), "replace")
    if kind == "refused_analysis":
        which = rng.choice(ANALYSIS_REFUSALS)
        if which == "merge_raw":
            raw = scene_form(s.scene) == "raw" and scene_n(s.scene) >= 33
            return ([] if raw else [("scene", ("synth", rng.choice((2049, 7000)), rng.randrange(1, 50), "raw"))]) + [("refused", which)]
        if which == "merge_with_sh":
            return pre + ([] if sh_now is not None else [("sh", (rng.randrange(1, 99), 0.0, 0.25, 0.5))]) + [("refused", which)]
        return pre + [("refused", which)]
    scope = rng.choice(SCOPES)
    if "selected" in scope and rng.random() < 0.7:
        pre = pre + [some]
    if "visible" in scope and rng.random() < 0.7:
        pre = pre + [("set_hidden", (rng.randrange(1, 99), rng.choice((0.2, 0.4))), "replace")]
    radius = h * rng.choice((0.8, 1.0, 1.3, 1.7))
    selop = rng.choice(SELOPS)
    if kind == "select_neighbours":
        lo, hi, cap = rng.choice(((0, 1, 4), (1, None, 16), (2, None, 64), (1, 3, 2)))
        return pre + [(kind, radius, lo, hi, cap, scope, selop)]
    if kind == "select_clusters":
        lo, hi = rng.choice(((0, 2), (2, None), (3, None), (1, 4)))
        return pre + [(kind, radius, lo, hi, rng.choice((0, 1, 3)), scope, selop)]
    if kind == "select_cluster_at":
        min_pts = rng.choice((0, 1, 2))
        seed = "largest"
        if rng.random() < 0.6:          # an index seed: a labelled splat of the scene as it will be, from the reference
            st, S, H = _evaluate(fold_ops(s, pre), oracle)
            lab = _analysis_refs()[1].Clusters(st.positions[:3 * st.n], radius, min_pts, scope_mask(scope, S, H)).labels
            labelled = np.flatnonzero(lab != 0xffffffff)
            if labelled.size:
                seed = int(labelled[rng.randrange(labelled.size)])
        return pre + [(kind, radius, seed, min_pts, scope, selop)]
    if kind == "select_knn":
        k, stat = rng.choice((1, 4, 8)), rng.choice(("kth", "mean"))
        if rng.random() < 0.3:          # the statistical outlier filter, its threshold a constant of the operation
            return pre + ([("sh", None)] if sh_now is not None else []) + [(kind, radius, k, "mean", 0.75 * radius, None, scope, "replace"), ("erase", False)]
        return pre + [(kind, radius, k, stat, 0.0, radius * rng.choice((0.6, 0.8)), scope, selop)]
    if kind == "merge_cells":
        no_sh = [("sh", None)] if sh_now is not None else []
        if rng.random() < 0.3:          # copies sit exactly on their originals: the most natural merge there is
            return pre + no_sh + [("set_selection", (rng.randrange(1, 99), 0.2), "replace"), ("duplicate", None), (kind, COINCIDENT, tuple(x for x in scope if x != "selected"))]
        return pre + no_sh + [(kind, h * rng.choice((0.5, 0.8, 1.2, 1.6)), scope)]
    if kind == "report":
        which = rng.choice(REPORTS)
        args = {"neighbours": (radius, rng.choice((4, 64)), scope), "clusters": (radius, rng.choice((0, 2)), scope),
                "knn": (radius, rng.choice((1, 8)), rng.choice(("kth", "mean")), scope), "cells": (radius, rng.choice((1, 8)), scope)}[which]
        return pre + [("report", which) + args]
    raise AssertionError(kind)


def fold_ops(state, ops):
    for op in ops:
        state = fold(state, op)
    return state


def walk(seed, steps, start=State(), kinds=KINDS, oracle=None):
    """A seeded random walk over the same operations with cheap States (<= 20 000 splats, <= 900 x 700).  The kinds are dealt like
    cards -- one shuffled deck after another -- so that a walk of twice as many steps as there are kinds and preludes holds every
    kind; walk(seed, k) is the first k steps of walk(seed, k + 1), so a failure at step k replays as walk(seed, k + 1).
    kinds: KINDS (the walks as they always were), or KINDS + EDIT_KINDS: the editing layer's kinds and its refusals join the deck
    (scenes then grow to at most MAX_GROWN splats).  Those steps depend on the scene -- a hide must hide something that shows --,
    so the walk needs the `oracle` (CPU) to ask `vacuous`, draws a kind's operations again up to eight times and leaves the kind
    to the next deck if all of them would check nothing.  With kinds of ANALYSIS_KINDS among them the analysis layer's kinds and
    refusals join the deck under the same rule (_gen_analysis: on rows scenes of at most MAX_ANALYSED splats), and the accumulators
    are reset in front of a merge as in front of MOVES_GEOMETRY."""
    rng = random.Random(seed)
    t, s = [], start
    if kinds is KINDS or tuple(kinds) == KINDS:
        while len(t) < steps:
            deck = list(KINDS)
            rng.shuffle(deck)
            for kind in deck:
                for op in _gen(kind, s, rng):
                    check = not (op[0] in KEEPS_FRAME and rng.random() < 0.3)
                    t.append(Step(op, check))
                    s = fold(s, op)
        return t[:steps]
    assert oracle is not None, "a walk over the editing layer asks the oracle which steps check something"
    analysis = any(k in ANALYSIS_KINDS for k in kinds)      # (the analysis layer's kinds and its refusals join the deck as the editing layer's did)
    while len(t) < steps:
        deck = list(kinds) + ["refused_edit"] + (["refused_analysis"] if analysis else [])
        rng.shuffle(deck)
        for kind in deck:
            for _ in range(8):
                if kind in ANALYSIS_KINDS or kind == "refused_analysis":
                    ops = _gen_analysis(kind, s, rng, oracle)
                else:
                    ops = _gen(kind, s, rng) if kind in KINDS else _gen_edit(kind, s, rng)
                s1, out = s, []
                for op in ops:
                    if s1.contrib and op[0] in MOVES_GEOMETRY + ("merge_cells",):
                        out.append(("contrib_reset",))   # (the accumulators describe frames of splats that are about to move)
                        s1 = fold(s1, out[-1])
                    if vacuous(s1, op, oracle) is not None:
                        out = None
                        break
                    out.append(op)
                    s1 = fold(s1, op)
                if out is not None:
                    break
            if out is None:
                continue
            for op in out:
                check = not ((op[0] in KEEPS_FRAME or op[0] in EDIT_KEEPS_FRAME or op[0] in ANALYSIS_KEEPS_FRAME) and rng.random() < 0.3)
                t.append(Step(op, check))
                s = fold(s, op)
    return t[:steps]


def describe(trace, upto=None):
    return "; ".join("%d:%s%s" % (i, " ".join(str(v) for v in st.op), "" if st.check else " (unchecked)")
                     for i, st in enumerate(trace[:upto]))


# ---------------------------------------------------------------------------------------------------------------------------
# Applying a State or an operation to a HIPRenderer
# ---------------------------------------------------------------------------------------------------------------------------
_rows_cache = {}


def scene_arrays(gh, recipe):
    """(rows, data, positions) of a recipe; data / positions (the packed form gsr_set_scene takes) only for raw recipes"""
    key = recipe
    if key not in _rows_cache:
        if len(_rows_cache) >= 16:
            _rows_cache.pop(next(iter(_rows_cache)))
        rows = gh.synth.config_rows(recipe[1]) if recipe[0] == "config" else gh.synth.synth_rows(recipe[1], recipe[2])
        data = pos = None
        if scene_form(recipe) == "raw":
            sc = gh.Scene()
            sc.setData(rows)
            data, pos = sc.data[:8 * sc.vertexCount].copy(), sc.positions
        _rows_cache[key] = (rows, data, pos)
    return _rows_cache[key]


def sh_arrays(gh, spec, n):
    """three half textures of 8 words per splat and the band indices of an SH spec for a scene of n splats"""
    seed, f0, f1, f2 = spec
    rng = np.random.default_rng(seed)
    band = np.array([int(f0 * n) - 1, int(f1 * n) - 1, int(f2 * n) - 1], dtype=np.int32)
    count = n - (int(band[0]) + 1)
    tex = []
    for _ in range(3):
        c = rng.standard_normal((max(count, 0) * 8, 2)) * 0.2
        tex.append(np.ascontiguousarray(gh.pack_half2x16(c[:, 0], c[:, 1]), dtype=np.uint32))
    return tex, band


def camera_of(gh, state, pose=None):
    return gh.orbit_camera(state.pose if pose is None else pose, 120, state.W, state.H, fx=0.59 * state.W)


def _load_scene(gh, r, recipe):
    rows, data, pos = scene_arrays(gh, recipe)
    if scene_form(recipe) == "rows":
        r.set_scene_rows(rows)
    else:
        r.set_raw_scene(data, pos)


def _transform(r, name, values):
    getattr(r, "scene_" + name)(list(values))


def _set_sh(gh, r, spec):
    if spec is None:
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        return
    tex, band = sh_arrays(gh, spec, r._n)
    if r._n - (int(band[0]) + 1) <= 0:      # (no splat carries SH: the call with count 0 clears the state, like None)
        r._check(r._L.gsr_set_scene_sh(r._ctx, None, None, None, 0, None))
        return
    r.set_sh(tex, band)


def _open_ring(r, ring):
    fmt, full, depth, step = ring
    if depth is None:
        r.open_delivery(3, fmt, full)
    else:
        r.open_delivery_depth(3, fmt, full, (0, 0, 0), depth, step, 0.1)


def build(gh, state, lib_path=None):
    """A context created from the State alone: same kind, same pinned knobs; it has done nothing else."""
    saved = {k: os.environ.get(k) for k, _ in state.knobs}
    try:
        for k, v in state.knobs:
            os.environ[k] = v
        r = gh.HIPRenderer(state.W, state.H, band=state.band, timing=state.timing, throughput=state.kind == "throughput", lib_path=lib_path)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        _build_scene(gh, r, state)
        if state.sh is not None:
            _set_sh(gh, r, state.sh)
        if state.fade != (False, 0.0):
            r.set_depth_fade(*state.fade)
        if state.hit_alpha != 0.5:
            r.set_hit_alpha(state.hit_alpha)
        if state.overlay is not None:
            _set_overlay(r, state.overlay)
        if state.ring is not None:
            _open_ring(r, state.ring)
        if state.ring_overlay:      # (the switch needs options when it is thrown; it stays when they go)
            if state.overlay is None:
                r.set_overlay((1.0, 0.5, 0.0), 0.5)
            r.delivery_set_overlay(True)
            if state.overlay is None:
                r.set_overlay(None)
    except Exception:
        r.dispose()
        raise
    return r


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


def _build_scene(gh, r, state):
    """The State's scene on a fresh context.  Without edits: the upload and the device's transforms, as ever.  With edits: the
    materialised arrays, selection and hidden words -- a capacity equal to n, no edit kernel, no growth -- and the contribution
    passes rendered again."""
    if not state.edits and state.contrib is None:
        _load_scene(gh, r, state.scene)
        for name, values in state.transforms:
            _transform(r, name, values)
        return
    O = _oracle()
    if not state.edits:
        _load_scene(gh, r, state.scene)
        for name, values in state.transforms:
            _transform(r, name, values)
        m = None
    else:
        m = materialise(state, O)
        if scene_form(state.scene) == "rows" and m.n:
            r.set_scene_arrays(m.data, m.positions, m.rotations, m.scales)
        else:                       # (a raw scene takes pickers and hides only: its arrays are the upload's)
            _load_scene(gh, r, state.scene)
            assert r.scene_count() == m.n
        if m.selection_words.any():
            r.set_selection(words=m.selection_words)
    if state.contrib is not None:
        _replay_contrib(gh, r, state, O)
    if m is not None and m.hidden_words.any():
        r.set_hidden(words=m.hidden_words)


def _replay_contrib(gh, r, state, O):
    """The accumulators of the State: every pass since the last reset rendered again under its pose, size, band and fade.  Rows
    appended since a pass did not exist for it: they are hidden while it is rendered again (a hidden splat is in no list, and the
    order of the others does not depend on it), and so is what was hidden then."""
    n = r.scene_count()
    r.contrib_reset()
    hid_any, cur_band, cur_fade = False, state.band, (False, 0.0)

    def frame_like(W, H, band, fade):
        nonlocal cur_band, cur_fade
        if (r.width, r.height) != (W, H):
            r.setSize(W, H)
            cur_band = None                     # (gsr_resize drops the band)
        if band != cur_band:
            r.set_band(*(band if band is not None else (0, 0)))
            cur_band = band
        if fade != cur_fade:
            r.set_depth_fade(*fade)
            cur_fade = fade

    for pose, W, H, band, fade, at in state.contrib:
        frame_like(W, H, band, fade)
        then = materialise(replace(state, edits=state.edits[:at]), O)
        assert then.n <= n
        hid = np.ones(n, dtype=bool)
        hid[:then.n] = _refs()[3].unpack(then.hidden_words, then.n)
        if hid.any() or hid_any:
            r.set_hidden(hid)
            hid_any = True
        r.set_camera(gh.orbit_camera(pose, 120, W, H, fx=0.59 * W))
        r.render_async()
        r.contrib_accumulate()
    r.sync()
    frame_like(state.W, state.H, state.band, (False, 0.0))
    if hid_any:
        r.set_hidden(None)


def _set_overlay(r, overlay):
    tint, mix, outline = overlay
    r.set_overlay(tint, mix)
    if outline is None:
        r.set_overlay_outline(None)
    else:
        rgb, alpha, threshold, width, side = outline
        r.set_overlay_outline(rgb, alpha, threshold, width, side)


def _frame(gh, r, state, pose=None, sync=False):
    r.set_camera(camera_of(gh, state, pose))
    r.render_async()
    if sync:
        r.sync()


def _refuse(gh, r, state, which):
    """one call the library must refuse; returns the error code it gave"""
    try:
        if which == "band_off_boundary":
            r.set_band(10, 50)
        elif which == "size_zero":
            r.setSize(0, 10)
        elif which == "timing_interval_zero":
            r.set_timing_interval(0)
        elif which == "edit_raw":                        # (edits need rotations / scales)
            r.scene_translate_selected((0.5, 0.0, 0.0))
        elif which == "erase_raw":
            r.scene_erase_selected()
        elif which == "rotate_selected_sh_follow":       # (the SH frame is one per scene: a partial rotation has none)
            r.set_sh_follow(True)
            try:
                r.scene_rotate_selected(QUAT)
            finally:
                r.set_sh_follow(False)
        elif which in ("grow_with_sh", "append_positions_differ"):
            add = _oracle().SceneState(gh.synth.synth_rows(3, 78))
            pos = add.positions + np.float32(1.0) if which == "append_positions_differ" else add.positions
            r.scene_append_arrays(add.data, pos, add.rotations, add.scales)
        else:
            rows = gh.synth.synth_rows(500, 77)
            sc = gh.Scene()
            sc.setData(rows)
            r.set_raw_scene(sc.data[:8 * 500], sc.positions + np.float32(1.0))
    except gh.GsplatError as e:
        return e.code
    raise AssertionError("the library accepted %s" % which)


def deliver_refused(gh, r):
    """gsr_deliver_frame_async in a State of overlay_ring_refuses: refused, and only in that way; returns the message"""
    try:
        r.deliver()
    except gh.GsplatError as e:
        assert e.code == GSR_ERR_ARG and "the options are off" in str(e), str(e)
        return str(e).split(": ", 1)[-1]
    raise AssertionError("the ring delivered an overlay without options")


def apply(gh, r, op, before, edited=False):
    """Perform `op` on the renderer, which is in State `before`.  Returns a dict of what the operation itself observed
    ({"overflowed": bool} for the overflow operations).  edited: the scene was edited since the renderer's last frame (a read-back
    of planes or picks is then refused, and only then)."""
    kind, a = op[0], op[1:]
    out = {}
    if kind == "camera":
        _frame(gh, r, before, a[0])                       # (in flight: whatever comes next finds it unsynchronised)
    elif kind == "same_pose":
        for _ in range(2):
            r.set_camera(camera_of(gh, before))
            r._check(r._L.gsr_render(r._ctx))             # the blocking entry point
    elif kind == "burst":
        for p in a:
            _frame(gh, r, before, p)
    elif kind == "sort_only":
        for k in range(a[0]):
            r.sort(camera_of(gh, before, (a[1] + k) % 120))
    elif kind == "readback":
        which = a[0]
        try:
            if which == "records":
                r.read_records()
            elif which == "keys":
                r.read_keys()
            elif which == "bin_lists":
                r.bin_lists()
            elif which == "work_items":
                r.work_items()
            elif which == "depth_index":
                r.lastDepthIndex()
            elif which == "read_depth":
                r.read_depth()
            elif which == "pick":
                r.pick([into_band(before, x, y) for x, y in ((before.W // 2, before.H // 2), (0, 0), (before.W - 1, before.H - 1))])
            else:
                r.stats()
        except gh.GsplatError as e:
            # the documented refusals: planes and picks of a frame need its bin lists, and the frame enqueued last was sort-only
            # (gsr_sort, or the whole permutation a band context sorts on demand for gsr_read_depth_index / gsr_read_keys); or, with
            # `edited` (the caller knows that the scene was edited since the last frame, through this context or another member
            # of its shared scene), the frame is gone until the next one is rendered
            ok = "sort-only" in str(e) or (edited and "no frame has been rendered yet" in str(e))
            assert which in ("read_depth", "pick") and e.code == GSR_ERR_ARG and ok, (which, str(e))
            out["refused"] = str(e)
    elif kind == "scene":
        _load_scene(gh, r, a[0])
    elif kind == "resize":
        r.setSize(a[0], a[1])
    elif kind == "band":
        r.set_band(a[0], a[1])
    elif kind == "sh":
        _set_sh(gh, r, a[0])
    elif kind in ("limit_box", "rotate", "translate", "scale"):
        _transform(r, kind, a[0])
    elif kind == "fade":
        r.set_depth_fade(a[0], a[1])
    elif kind == "hit_alpha":
        r.set_hit_alpha(a[0])
    elif kind == "depth_async":
        _frame(gh, r, before)
        r.depth_async()                                   # behind the frame, no host wait
        if a[0]:
            r.read_depth()                                # the cached planes; the next frame must not get them
    elif kind == "timing_interval":
        r.set_timing_interval(a[0])
    elif kind == "overflow_sync":
        r.set_list_capacity(a[0])                         # the next frame (the step's own) may not fit: gsr_sync repairs it
    elif kind == "overflow_async":
        r.set_list_capacity(a[0])
        dropped = r.stats()["dropped_frames"]
        for p in a[1:]:
            _frame(gh, r, before, p)
        try:
            r.sync()
            out["overflowed"] = False
        except gh.GsplatError as e:
            assert e.code == GSR_ERR_OVERFLOW, str(e)
            out["overflowed"] = True
        r.sync()                                          # reported once
        assert (r.stats()["dropped_frames"] > dropped) == out["overflowed"]
        assert not r.overflow_pending()
    elif kind == "ring_open":
        _open_ring(r, tuple(a))
    elif kind == "ring_close":
        r.close_delivery()
    elif kind == "deliver":
        _frame(gh, r, before)
        if overlay_ring_refuses(before):
            out["refused"] = deliver_refused(gh, r)
            return out
        k = r.deliver()
        got = r.acquire(k)
        assert got[0] == k
        r.release(k)
    elif kind == "refused" and a[0] in ANALYSIS_REFUSAL_TEXTS:
        out["code"], out["message"] = _refuse_analysis(gh, r, a[0])
        assert out["code"] == GSR_ERR_ARG and ANALYSIS_REFUSAL_TEXTS[a[0]] in out["message"], (a[0], out)
    elif kind == "refused":
        out["code"] = _refuse(gh, r, before, a[0])
    else:
        _apply_editing(gh, r, op, before, out)
    return out


def _apply_editing(gh, r, op, before, out):
    kind, a = op[0], op[1:]
    if kind == "select_box":
        r.select_box(a[0], a[1])
    elif kind == "select_region":                         # centre mode, from the frame of the State's pose
        _frame(gh, r, before)
        r.select_region(a[0], mask_of(a[1]), "centre", a[2])
    elif kind == "set_selection":
        r.set_selection(None if a[0] is None else spec_set(a[0], r._count()), a[1])
    elif kind == "invert_selection":
        r.invert_selection()
    elif kind == "select_attr":
        r.select_attr(a[0], a[1], a[2], a[3], a[4])
    elif kind == "select_hidden":
        r.select_hidden(a[0])
    elif kind == "select_contrib":
        r.select_contrib(a[0], a[1], a[2])
    elif kind == "hide":
        r.hide_selected(a[0])
    elif kind == "set_hidden":
        r.set_hidden(None if a[0] is None else spec_set(a[0], r._count()), a[1])
    elif kind == "edit":
        what, args, pivot = a
        if what == "translate":
            r.scene_translate_selected(args)
        elif what == "rgba":
            r.scene_set_rgba_selected(args[0], args[1])
        else:
            getattr(r, "scene_%s_selected" % what)(args, pivot)
    elif kind == "reserve":
        r.scene_reserve(a[0])
    elif kind == "duplicate":
        cap = r.scene_capacity()
        first, count = r.scene_duplicate_selected()
        out["count"] = count
        if a[0]:                                          # the trace says on which side of the capacity this copy falls
            assert count and (r.scene_capacity() == cap) == (a[0] == "fit"), (op, cap, r.scene_capacity(), first, count)
    elif kind == "append_arrays":
        add = _oracle().SceneState(recipe_rows(("synth", a[0], a[1], "rows")))
        r.scene_append_arrays(add.data, add.positions, add.rotations, add.scales)
    elif kind == "erase":
        n0 = r.scene_count()
        n1 = r.scene_erase_selected(keep=a[0])
        assert 0 < n1 < n0, (op, n0, n1)                  # (the traces' erases all remove something and leave something)
    elif kind == "overlay":
        if a[0] is None:
            r.set_overlay(None)
        else:
            _set_overlay(r, a)
    elif kind == "ring_overlay":
        r.delivery_set_overlay(a[0])
    elif kind == "contrib_reset":
        r.contrib_reset()
    elif kind == "contrib_pass":
        r.set_camera(camera_of(gh, before))
        r._check(r._L.gsr_render(r._ctx))                 # the blocking entry point: a frame that did not fit is rendered again
        r.contrib_accumulate()
    elif kind == "select_neighbours":
        radius, lo, hi, cap, scope, selop = a
        out["selected"], out["info"] = r.select_neighbours(radius, lo, hi, cap, scope, selop)
    elif kind == "select_clusters":
        radius, lo, hi, min_pts, scope, selop = a
        out["selected"], out["info"] = r.select_clusters(radius, lo, hi, min_pts, scope, selop)
    elif kind == "select_cluster_at":
        radius, seed, min_pts, scope, selop = a
        out["selected"], out["info"] = r.select_cluster_at(radius, seed, min_pts, scope, selop)
    elif kind == "select_knn":
        radius, k, stat, lo, hi, scope, selop = a
        out["selected"], out["info"] = r.select_knn(radius, k, stat, lo, hi, scope, selop)
    elif kind == "merge_cells":
        n0 = r.scene_count()
        n1, out["info"] = r.scene_merge_cells(a[0], a[1])
        assert 2 <= n1 < n0 and n1 == r.scene_count(), (op, n0, n1)      # (the traces' merges all merge something and leave something)
    elif kind == "report":
        out["report"] = report(r, a)
    else:
        raise AssertionError(op)


def report(r, a):
    """one of the read-only calls, ("neighbours" | "clusters" | "knn" | "cells", arguments as the operation holds them): what it returned"""
    which = a[0]
    if which == "neighbours":
        return r.neighbours(a[1], a[2], a[3])
    if which == "clusters":
        return r.clusters(a[1], a[2], a[3])
    if which == "knn":
        return r.knn(a[1], a[2], a[3], a[4])
    if which == "cells":
        return r.cells(a[1], a[2], a[3], leaders=True)
    raise AssertionError(a)


def _refuse_analysis(gh, r, which):
    """one call of the analysis layer the library must refuse; returns (code, message).  The calls go to the C ABI where the Python
    layer would stop them first (cap, k)."""
    L, ctx = r._L, r._ctx
    inf, nan = float("inf"), float("nan")
    if which in ("merge_raw", "merge_with_sh"):
        rc = L.gsr_scene_merge_cells(ctx, 0.25, 0, 0, None, None)
    elif which == "budget_of_one":
        rc = L.gsr_select_neighbours(ctx, 0.25, 8, 0, 1, 0, 9, 0, None, None)
    elif which == "cell_not_finite":
        rc = L.gsr_scene_merge_cells(ctx, inf, 0, 0, None, None)
    elif which == "cell_not_positive":
        rc = L.gsr_cells(ctx, 0.0, 8, 0, 0, None, 0, None, None)
    elif which == "radius_not_finite":
        rc = L.gsr_select_knn(ctx, nan, 4, 0, 0, 1, 0.0, 1.0, 0, None, None)
    elif which == "radius_not_positive":
        rc = L.gsr_select_clusters(ctx, -0.25, 0, 0, 0, 0, 4, 0, None, None)
    elif which == "cap_out_of_range":
        rc = L.gsr_select_neighbours(ctx, 0.25, 4096, 0, 0, 0, 1, 0, None, None)
    elif which == "k_out_of_range":
        rc = L.gsr_knn(ctx, 0.25, 33, 0, 0, 1, None, None, None, None, 0, None, None)
    else:
        raise AssertionError(which)
    if rc == 0:
        raise AssertionError("the library accepted %s" % which)
    return rc, L.gsr_last_error(ctx).decode()
