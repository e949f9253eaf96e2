"""tests/depth_exchange_reference.py against itself: cutting a delivered plane into the ranks' depth sections and assembling them
is the identity, every sample has exactly one owner, and the layout keeps the alignments the kernels rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_delivery_reference as D   # noqa: E402
import depth_exchange_reference as X   # noqa: E402

from gsplat_hip import bands   # noqa: E402

SIZES = [(640, 480), (1920, 1080), (3840, 2160), (1000, 37), (333, 201), (1001, 3), (33, 1), (2049, 65)]
WORLDS = [1, 2, 3, 8, 16]


def _hit(W, H, seed):
    rng = np.random.default_rng(seed)
    hit = rng.uniform(0.01, 50.0, size=(H, W)).astype(np.float32)
    hit[rng.random((H, W)) < 0.3] = np.inf          # no hit
    hit[rng.random((H, W)) < 0.05] = np.float32(0.02)   # in front of near
    return hit


def _plane(hit, step, fmt):
    s = D.subsample(hit, step)
    return s if fmt == "f32" else D.quantise_u16(s, 0.1)


def _edge_sets(W, world):
    """the equal split, and where the grid allows it a split whose widest band is not the last"""
    out = [bands.band_edges(W, world)]
    nbx = -(-W // 32)
    if world >= 2 and nbx >= world + 1:
        cuts = [0, nbx - (world - 1)] + [nbx - (world - 1) + k for k in range(1, world)]   # rank 0 takes the slack
        out.append([(min(a * 32, W), min(b * 32, W)) for a, b in zip(cuts[:-1], cuts[1:])])
    return out


@pytest.mark.parametrize("fmt", ["f32", "u16"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("world", WORLDS)
def test_assembly_is_the_identity_and_every_sample_has_one_owner(world, step, fmt):
    widest_first = 0
    for k, (W, H) in enumerate(SIZES):
        plane = _plane(_hit(W, H, 100 * world + k), step, fmt)
        Wd, Hd = D.plane_size(W, H, step)
        assert plane.shape == (Hd, Wd)
        for edges in _edge_sets(W, world):
            widths = [b - a for a, b in edges]
            widest_first += widths[0] > widths[-1]
            lay = X.layout(W, H, edges, step, fmt)
            assert (lay["Wd"], lay["Hd"]) == (Wd, Hd)
            # alignment: the section and every row of it start on 16 bytes; the slab is whole 16 bytes
            assert lay["offset"] % 16 == 0 and (lay["stride"] * lay["sample_bytes"]) % 16 == 0 and lay["slab_bytes"] % 16 == 0
            assert lay["offset"] >= X.colour_bytes(X.slab_width(edges), H) and lay["offset"] - X.colour_bytes(X.slab_width(edges), H) < 16
            se = X.sample_edges(edges, step)
            # disjoint, in order, covering [0, Wd) (empty bands of surplus ranks own nothing)
            assert se[0][0] == 0 and max(b for _, b in se) >= Wd
            for (a0, b0), (a1, b1) in zip(se[:-1], se[1:]):
                assert min(b0, Wd) <= a1 or a1 >= Wd, (edges, step)
            assert max(min(b, Wd) - a for a, b in se) <= lay["stride"]
            secs = [X.section(plane, edges, q, step, fmt) for q in range(world)]
            for sec in secs:
                assert sec.shape == (Hd, lay["stride"]) and sec.nbytes == lay["section_bytes"]
            back, owners = X.assemble(secs, Wd, edges, step)
            assert np.array_equal(owners, np.ones_like(owners)), (W, H, edges)
            assert back.tobytes() == plane.tobytes(), (W, H, edges)
            # behind a band's samples a section holds zeros
            for sec, (a, b) in zip(secs, se):
                assert not sec[:, max(min(b, Wd) - a, 0):].any()
    if world >= 2:
        assert widest_first, "no case with the widest band in front"


def test_sizes_cover_the_ragged_cases():
    assert any(W % 32 for W, _ in SIZES) and any(W % 2 and H % 2 for W, H in SIZES) and any(W % 32 == 0 for W, _ in SIZES)


def test_documented_numbers():
    """3840 x 2160 in eight bands"""
    edges = bands.band_edges(3840, 8)
    assert X.slab_width(edges) == 480
    lay = X.layout(3840, 2160, edges, 2, "u16")
    assert lay == {"Wd": 1920, "Hd": 1080, "stride": 240, "offset": 4147216, "section_bytes": 518400, "slab_bytes": 4665616, "sample_bytes": 2}
    lay = X.layout(3840, 2160, edges, 1, "f32")
    assert lay["stride"] == 480 and lay["section_bytes"] == 4147200 and lay["slab_bytes"] == 4147216 + 4147200
