"""tests/append_reference.py pinned against itself and the oracle's SceneState: a duplicate of everything is the state concatenated
with itself, duplicate-then-erase gives the state back bit for bit, a NaN and a -0.0 travel as bits, and the capacity rule."""
import copy

import numpy as np
import pytest

import append_reference as ar

N = 3000
Q0, S0 = (0.1, -0.3, 0.2, 0.9273618495495703), (1.25, 0.8, 1.1)
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


def test_duplicate_of_everything_is_the_state_concatenated_with_itself(oracle):
    st = _state(oracle)
    before = _bits(st)
    first, count = ar.duplicate(st, np.ones(N, dtype=bool))
    assert (first, count, st.n) == (N, N, 2 * N)
    for f in FIELDS:
        assert np.array_equal(_bits(st)[f], np.concatenate([before[f], before[f]])), f


def test_rows_below_n_keep_their_bits_and_row_n_plus_j_is_row_idx_j(oracle):
    st = _state(oracle)
    before = _bits(st)
    sel = _mask(N)
    idx = np.flatnonzero(sel)
    first, count = ar.duplicate(st, sel)
    assert first == N and count == idx.size and st.n == N + idx.size
    for f, k in zip(FIELDS, (8, 3, 4, 3)):
        after = _bits(st)[f].reshape(-1, k)
        assert np.array_equal(after[:N], before[f].reshape(-1, k)), f
        assert np.array_equal(after[N:], before[f].reshape(-1, k)[idx]), f
    assert np.array_equal(ar.selection_after(st.n, first, count), np.arange(st.n) >= N)


@pytest.mark.parametrize("kind", ("mask", "all", "none", "one"))
def test_duplicate_then_erase_the_new_selection_gives_the_state_back(oracle, kind):
    st = _state(oracle)
    before = _bits(st)
    sel = {"mask": _mask(N), "all": np.ones(N, bool), "none": np.zeros(N, bool), "one": np.arange(N) == N - 1}[kind]
    first, count = ar.duplicate(st, sel)
    assert count == int(sel.sum())
    assert ar.erase(st, ar.selection_after(st.n, first, count)) == N
    for f in FIELDS:
        assert np.array_equal(_bits(st)[f], before[f]), f


def test_a_nan_row_and_a_negative_zero_are_copied_as_bits(oracle):
    st = _state(oracle)
    nan, neg0 = np.uint32(0x7fc01234), np.uint32(0x80000000)   # a NaN with a payload
    for row, word in ((700, nan), (701, neg0)):
        st.positions.view(np.uint32)[3 * row + 1] = word
        st.data[8 * row + 1] = word
    sel = np.zeros(N, dtype=bool)
    sel[[5, 700, 701]] = True
    first, _ = ar.duplicate(st, sel)
    pos = st.positions.view(np.uint32)
    assert pos[3 * (first + 1) + 1] == nan and st.data[8 * (first + 1) + 1] == nan
    assert pos[3 * (first + 2) + 1] == neg0 and st.data[8 * (first + 2) + 1] == neg0


def test_append_selected_and_arrays_read_the_other_state_and_leave_it_alone(oracle):
    dst, src = _state(oracle, 1023), _state(oracle, 257, seed=5)
    before_dst, before_src = _bits(dst), _bits(src)
    sel = _mask(257)
    want = copy.deepcopy(dst)
    sub_first, sub_count = ar.append_selected(dst, src, sel)
    assert (sub_first, sub_count) == (1023, int(sel.sum()))
    for f, k in zip(FIELDS, (8, 3, 4, 3)):
        assert np.array_equal(_bits(src)[f], before_src[f]), f
        assert np.array_equal(_bits(dst)[f].reshape(-1, k)[:1023], before_dst[f].reshape(-1, k)), f
        assert np.array_equal(_bits(dst)[f].reshape(-1, k)[1023:], before_src[f].reshape(-1, k)[sel]), f
    idx = np.flatnonzero(sel)
    first, count = ar.append_arrays(want, src.data.reshape(-1, 8)[idx], src.positions.reshape(-1, 3)[idx], src.rotations.reshape(-1, 4)[idx],
                                    src.scales.reshape(-1, 3)[idx])
    assert (first, count) == (sub_first, sub_count)
    for f in FIELDS:
        assert np.array_equal(_bits(want)[f], _bits(dst)[f]), f


def test_state_beside_the_arrays_and_the_capacity_rule():
    hid = np.array([1, 0, 1], dtype=bool)
    assert ar.hidden_after(hid, 2).tolist() == [True, False, True, False, False]
    w, p, x = ar.contrib_after((np.array([5, 6], np.uint64), np.array([.5, .25], np.float32), np.array([7, 8], np.uint32)), 3)
    assert w.tolist() == [5, 6, 0, 0, 0] and w.dtype == np.uint64 and p.dtype == np.float32 and x.tolist() == [7, 8, 0, 0, 0]
    assert ar.capacity_after(100, 100) == 100 and ar.capacity_after(100, 101) == 150 and ar.capacity_after(100, 400) == 400
    assert ar.capacity_after(31, 62) == 62 and ar.capacity_after(62, 93) == 93 and ar.capacity_after(93, 124) == 139
    assert ar.capacity_after(ar.MAX_ROWS - 1, ar.MAX_ROWS) == ar.MAX_ROWS
