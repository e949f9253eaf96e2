"""What the source-text tests of the passes behind the frame (test_depth_reference.py, test_contrib_abi.py, test_overlay_abi.py)
assert about the one walk of k_depth_walk.h: k_depth.hip and k_overlay.hip instantiate its skeleton; k_contrib.hip keeps a loop of its own
(its flush and barrier scheme; through the skeleton it measured slower, profiles/second_walk_ab.txt) over the skeleton's helpers."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsplat.js_amd", "csrc")


def walk_sites_are_checked(src, unit, bounds, passname):
    """the four check sites every walk shares are in the skeleton of k_depth_walk.h, under the same numbers for every unit, and
    `src` (the text of k_<unit>.hip) forwards them to its own counters and instantiates the skeleton with them; passname None: the
    unit keeps its own chunk loop (k_contrib), takes sites 0 - 2 from the helpers and checks site 3, the LDS cell, itself"""
    walk = re.sub(r"//.*", "", open(os.path.join(CSRC, "k_depth_walk.h")).read())
    assert re.search(r"WALK_SITE_BIN = 0, WALK_SITE_LIST = 1, WALK_SITE_SPLAT = 2, WALK_SITE_CELL = 3;", walk)
    geometry = walk[walk.index("WalkBin walk_bin("):walk.index("uint32_t walk_list_entry(")]
    entry = walk[walk.index("uint32_t walk_list_entry("):walk.index("struct WalkStage")]
    loop = walk[walk.index("void walk_bin_list("):]
    assert "Bounds::bound(WALK_SITE_BIN, bin," in geometry and geometry.count("Bounds::bound(WALK_SITE_LIST, a.bin_start[") == 2
    assert "Bounds::bound(WALK_SITE_LIST, e, a.capacity)" in entry and "Bounds::bound(WALK_SITE_SPLAT, a.list[e], a.nsplats)" in entry
    assert "min(a.list[e], a.nsplats - 1u)" in entry
    assert "walk_list_entry<Pass>(a, e)" in loop and "Pass::bound(WALK_SITE_CELL, cell, DEPTH_CHUNK)" in loop
    assert loop.index("Pass::bound(WALK_SITE_CELL") < loop.index("s_a[cell]")            # checked in front of the read
    code = re.sub(r"//.*", "", src)
    assert '#include "k_depth_walk.h"' in src
    assert re.search(r"struct %s \{\s*static __device__ __forceinline__ void bound\(int site, unsigned long long idx, unsigned long long limit\) "
                     r"\{ GSR_BOUND\(%s, site, idx, limit\); \}" % (bounds, unit), code)
    assert "walk_bin<%s>(a, g, blockIdx.x)" % bounds in code
    if passname is None:
        assert "walk_list_entry<%s>(a, e)" % bounds in code and "walk_bin_list" not in code
        assert code.index("GSR_BOUND(%s, WALK_SITE_CELL, cell, DEPTH_CHUNK);" % unit) < code.index("s_a[cell]")   # checked in front of the read
        return
    assert re.search(r"struct %s : %s\b" % (re.escape(passname), bounds), code)
    assert "walk_bin_list<SKIP>(st, a, w, cam," in code
    assert "__shared__ WalkStage st;" in code


def walk_is_stated_once():
    """the per-fragment arithmetic and the structure of the walk are in k_depth_walk.h and in no unit"""
    walk = open(os.path.join(CSRC, "k_depth_walk.h")).read()
    for fn in ("struct DepthEntry", "DepthEntry depth_entry(", "float depth_weight(", "float depth_row_u(", "float depth_row_w(", "uint32_t depth_tile_reach("):
        assert fn in walk, fn
    walk_code = re.sub(r"//.*", "", walk)
    for fn in ("depth_entry(a.rec", "depth_tile_reach(en, cx, cy, w.binX0, w.binY0)", "struct WalkStage", "struct WalkBin", "void walk_bin_list(", "bool walk_frame_unfit("):
        assert fn in walk_code, fn
    # the structure of the walk is stated once: the staging arrays, the chunk loop, the ballot loop, the broadcast re-read and the
    # bin geometry are the header's and no unit's
    structure = (r"\bs_a\b", r"\bs_b\b", r"\bs_tiles\b", r"\+= DEPTH_CHUNK", r"c0 \+ \(uint32_t\)__builtin_ctzll\(bal\)", r"\bbin_start\b", r"\* TILE\b", r"\+ 0\.5f",
                 r"depth_tile_reach\(", r"\ben\.ncu = ")
    for pattern in structure:
        assert re.search(pattern, walk_code), pattern
    assert len(re.findall(r"\+= DEPTH_CHUNK", walk_code)) == 1 and len(re.findall(r"__ballot\(", walk_code)) == 1
    # ... narrowed for k_contrib.hip, which keeps the chunk loop (staging, ballot loop, re-read) beside its flush: the bin geometry, the
    # list range and the clamped entry read are still the helpers' and not restated there
    own_loop = (r"\bbin_start\b", r"\* TILE\b", r"\+ 0\.5f", r"a\.list\[", r"a\.nsplats")
    for name in ("k_depth.hip", "k_contrib.hip", "k_overlay.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert '#include "k_depth_walk.h"' in src, name
        for fn in ("depth_weight(", "depth_row_u(", "depth_row_w(", "walk_bin<"):
            assert fn in src, (name, fn)
        assert "exp2f" not in src and "struct DepthEntry" not in src, name          # used, never restated
        code = re.sub(r"//.*", "", src)
        if name == "k_contrib.hip":
            for fn in ("walk_list_entry<ContribBounds>(a, e)", "depth_entry(a.rec", "depth_tile_reach(en,", "walk_launch("):
                assert fn in code, fn
            assert len(re.findall(r"\+= DEPTH_CHUNK", code)) == 1 and "walk_bin_list" not in code
            for pattern in own_loop:
                assert not re.search(pattern, code), (name, pattern)
            continue
        assert "walk_bin_list<SKIP>(" in code, name
        if name == "k_overlay.hip":
            # the one exemption: the TRIM pre-pass over list[] and the mask, which the issue leaves in the unit, strides by chunks too;
            # it stages nothing and visits nothing
            trim = code[code.index("if constexpr (TRIM) {"):code.index("end = w.begin + min(s_last, w.end - w.begin);")]
            assert len(re.findall(r"\+= DEPTH_CHUNK", trim)) == 1 and "walk_list_entry<OverlayBounds>(a, e)" in trim
            code = code.replace(trim, "")
        for pattern in structure:
            assert not re.search(pattern, code), (name, pattern)
    # k_pick keeps its own loop and takes the geometry, the range and the clamped read from the same helpers
    pick = open(os.path.join(CSRC, "k_depth.hip")).read()
    pick = pick[pick.index("void k_pick("):pick.index("void k_depth_fill(")]
    for fn in ("walk_frame_unfit(a.overflow, a.invalid)", "walk_bin<DepthBounds>(a, g,", "walk_list_entry<DepthBounds>(a, e)", "depth_entry(", "base += WAVE"):
        assert fn in pick, fn
