"""tests/edit_reference.py pinned against the oracle it is built from: with everything selected it IS SceneState's transform, rows
outside the selection keep their bits, a pivot is the three explicit steps, and the box handles the empty set, a NaN and +-0."""
import copy

import numpy as np
import pytest

import edit_reference as er

N = 3000
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
Q, T, S, PIVOT = (-0.2, 0.5, 0.1, 0.8366600265340756), (0.25, -0.5, 1.0), (0.9, 1.2, 1.05), (0.3, -0.7, 1.9)
OPS = (("translate", T), ("rotate", Q), ("scale", S))
FIELDS = ("data", "positions", "rotations", "scales")


def _state(oracle, n=N, seed=17):
    import gsplat_hip as gh
    st = oracle.SceneState(gh.synth.synth_rows(n, seed))
    st.rotate(Q0)
    st.scale(S0)
    return st


def _bits(st):
    return {f: getattr(st, f).view(np.uint32).copy() for f in FIELDS}


def _mask(n):
    i = np.arange(n)
    return (7 * i + 3) % 5 < 2


@pytest.mark.parametrize("op, args", OPS)
def test_everything_selected_without_a_pivot_is_the_oracles_transform(oracle, op, args):
    a, b = _state(oracle), _state(oracle)
    getattr(a, op)(args)
    er.apply(b, np.ones(N, dtype=bool), op, args)
    for f in FIELDS:
        assert np.array_equal(_bits(a)[f], _bits(b)[f]), f


@pytest.mark.parametrize("op, args", OPS)
@pytest.mark.parametrize("pivot", (None, PIVOT))
def test_unselected_rows_keep_their_bits_and_selected_rows_are_the_sub_scenes(oracle, op, args, pivot):
    st = _state(oracle)
    before = _bits(st)
    sel = _mask(N)
    sub = er.sub_state(st, np.flatnonzero(sel))
    if pivot is not None:
        sub.translate([-v for v in pivot])
    getattr(sub, op)(args)
    if pivot is not None:
        sub.translate(pivot)
    er.apply(st, sel, op, args, pivot)
    after = _bits(st)
    for f, k in zip(FIELDS, (8, 3, 4, 3)):
        assert np.array_equal(after[f].reshape(-1, k)[~sel], before[f].reshape(-1, k)[~sel]), f
        assert np.array_equal(after[f].reshape(-1, k)[sel], getattr(sub, f).view(np.uint32).reshape(-1, k)), f
    changed = (after["positions"].reshape(-1, 3)[sel] != before["positions"].reshape(-1, 3)[sel]).any()
    assert changed


def test_a_pivot_is_not_the_operation_alone_and_zero_is_not_none(oracle):
    a, b, c = _state(oracle), _state(oracle), _state(oracle)
    sel = _mask(N)
    er.apply(a, sel, "rotate", Q, None)
    er.apply(b, sel, "rotate", Q, PIVOT)
    assert not np.array_equal(a.positions.view(np.uint32), b.positions.view(np.uint32))
    assert np.array_equal(a.rotations.view(np.uint32), b.rotations.view(np.uint32))   # the translate steps move centres only
    # pivot (0, 0, 0) turns a -0.0 coordinate into +0.0; no pivot keeps it
    c.positions[0:3] = np.float32(-0.0)
    c.data[0:3] = c.positions[0:3].view(np.uint32)
    d = copy.deepcopy(c)
    one = np.zeros(N, dtype=bool)
    one[0] = True
    er.apply(c, one, "scale", (1.0, 1.0, 1.0), None)
    er.apply(d, one, "scale", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert c.positions[:3].view(np.uint32).tolist() == [0x80000000] * 3
    assert d.positions[:3].view(np.uint32).tolist() == [0] * 3


def test_paint_writes_the_masked_bytes_of_the_selected_words_only(oracle):
    st = _state(oracle)
    before = _bits(st)["data"].reshape(-1, 8)
    sel = _mask(N)
    er.paint(st, sel, 0x80112233, 0xff000000)
    after = st.data.reshape(-1, 8)
    assert np.array_equal(after[:, :7], before[:, :7]) and np.array_equal(after[~sel, 7], before[~sel, 7])
    assert np.array_equal(after[sel, 7], (before[sel, 7] & 0x00ffffff) | 0x80000000)
    er.paint(st, sel, 0x80112233, 0x00ffffff)
    assert (st.data.reshape(-1, 8)[sel, 7] == 0x80112233).all()


def test_bounds_of_the_empty_set_a_nan_and_signed_zeros():
    pos = np.array([[1, 2, 3], [-4, 5, 0.5], [np.nan, 9, -7], [0.0, -0.0, 2]], dtype=np.float32)
    count, mn, mx = er.bounds(pos, np.zeros(4, dtype=bool))
    assert count == 0 and np.all(mn == np.inf) and np.all(mx == -np.inf) and mn.dtype == np.float32
    count, mn, mx = er.bounds(pos, np.array([1, 1, 1, 0], dtype=bool))
    assert count == 3 and mn.tolist() == [-4, 2, -7] and mx.tolist() == [1, 9, 3]     # the NaN is counted, its row's other coordinates enter
    count, mn, mx = er.bounds(pos, np.array([0, 0, 1, 0], dtype=bool))
    assert count == 1 and mn[0] == np.inf and mx[0] == -np.inf and mn[1] == 9 and mx[2] == -7
    count, mn, mx = er.bounds(pos, np.array([0, 0, 0, 1], dtype=bool))
    assert count == 1 and mn[0] == 0 and mx[1] == 0 and mn[1] == 0                     # +-0 compare equal
