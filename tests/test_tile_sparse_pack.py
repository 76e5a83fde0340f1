"""CPU tests of the tile-sparse view's packing routine (csrc/wrnn_abi.hip, `tile_sparse_pack`: what wrnn_pack_create runs on the six prunable matrices of a
generic pack for WRNN_ALGO_TILE_SPARSE), through the host-only `wrnn_debug_tile_sparse_pack` on numpy matrices.  The layout is the one
include/wavernn_amd.h documents and csrc/wrnn_tile_sparse.hip reads: per block row of 16 rows a list of surviving columns in groups of 16,
cols [group][kq][e] and vals [group][lane][e] for list entry 16 group + 4 e + kq.  No HIP device is needed."""
import numpy as np
import pytest

from test_planner_table import L      # noqa: F401  (the library fixture: builds the library when it is missing)


def _pack(W, gates):
    from wavernn_amd import _lib
    return _lib.tile_sparse_pack_host(W, gates)


def _lists(pk, rows):
    """The packed view decoded: per block row (columns [n], values [16, n], padded columns, padded values)."""
    out = []
    for br in range(rows // 16):
        g0, n = (int(v) for v in pk['tab'][br])
        ng = (n + 15) // 16
        cols, vals = np.zeros(16 * ng, np.int64), np.zeros((16, 16 * ng), np.float32)
        for g in range(ng):
            for kq in range(4):
                for e in range(4):
                    k = 16 * g + 4 * e + kq
                    cols[k] = pk['cols'][g0 + g, kq, e]
                    vals[:, k] = pk['vals'][g0 + g, 16 * kq:16 * kq + 16, e]
        out.append((cols[:n], vals[:, :n], cols[n:], vals[:, n:]))
    return out


def _scatter(pk, rows, K):
    W = np.zeros((rows, K), np.float32)
    for br, (cols, vals, _, _) in enumerate(_lists(pk, rows)):
        W[16 * br:16 * br + 16, cols] = vals
    return W


def _pruned(seed, H, K, gates, sparsity):
    from wavernn_amd.prune import block_mask
    W = np.random.RandomState(seed).standard_normal((gates * H, K)).astype(np.float32)
    return np.where(block_mask(W, sparsity, gates=gates) != 0, W, np.float32(0))       # (W * mask would leave -0.0 in the pruned blocks)


@pytest.mark.parametrize('H,K,gates,sparsity', [(32, 37, 3, 0.9), (144, 149, 3, 0.75), (80, 85, 1, 0.75), (256, 288, 1, 0.95), (48, 53, 3, 0.5)])
def test_a_block_pruned_matrix_round_trips_bit_for_bit(L, H, K, gates, sparsity):
    W = _pruned(3, H, K, gates, sparsity)
    pk = _pack(W, gates)
    assert np.array_equal(_scatter(pk, gates * H, K).view(np.uint32), W.view(np.uint32))
    nz = np.abs(W).reshape(gates * H // 16, 16, K).max(axis=1) > 0
    assert pk['kept'] == int(nz.sum()) and pk['total'] == gates * H // 16 * K
    groups = 0
    for br, (cols, vals, pad_cols, pad_vals) in enumerate(_lists(pk, gates * H)):
        assert np.array_equal(cols, np.flatnonzero(nz[br]))                       # every surviving column, ascending
        assert int(pk['tab'][br, 0]) == groups                                    # the lists lie one behind the other, in whole groups
        groups += (len(cols) + 15) // 16
        assert len(pad_cols) == -len(cols) % 16
        assert np.all(pad_vals.view(np.uint32) == 0)                              # padding: +0.0f ...
        assert np.all((pad_cols >= 0) & (pad_cols < K))                           # ... at a valid column,
        assert len(cols) == 0 or np.all(pad_cols == cols[-1])                     # the last surviving one
    assert groups == pk['cols'].shape[0] == pk['vals'].shape[0]


def test_empty_and_full_block_rows(L):
    K = 37
    W = _pruned(4, 32, K, 1, 0.9)
    W[0:16] = 0                                                   # block row 0: empty
    W[16:32] = np.random.RandomState(5).uniform(0.5, 1.0, (16, K))  # block row 1: every column
    pk = _pack(W, 1)
    (c0, v0, p0, _), (c1, v1, p1, pv1) = _lists(pk, 32)
    assert len(c0) == 0 and len(p0) == 0 and int(pk['tab'][0, 1]) == 0            # an empty list has no group at all
    assert np.array_equal(c1, np.arange(K)) and np.array_equal(v1, W[16:32])
    assert len(p1) == 48 - K and np.all(p1 == K - 1) and np.all(pv1 == 0)
    assert np.array_equal(_scatter(pk, 32, K), W)
    # one surviving VALUE keeps its block: the column is listed with its fifteen zeros
    W = np.zeros((16, 8), np.float32)
    W[11, 5] = -2.5
    pk = _pack(W, 1)
    (c, v, _, _), = _lists(pk, 16)
    assert list(c) == [5] and v[11, 0] == -2.5 and np.count_nonzero(v) == 1 and (pk['kept'], pk['total']) == (1, 8)
    # -0.0 is a zero: a block of them is pruned (`W * mask` leaves such blocks), one beside a non-zero value survives as it is
    W = np.full((16, 3), -0.0, np.float32)
    W[4, 1] = 7.0
    pk = _pack(W, 1)
    (c, v, _, _), = _lists(pk, 16)
    assert list(c) == [1] and pk['kept'] == 1 and np.array_equal(v[:, 0].view(np.uint32), W[:, 1].view(np.uint32))


def test_gate_boundaries_are_block_row_boundaries(L):
    """3 x H rows with K = H + A, A = 5: block row b is rows 16 b .. 16 b + 15, so gate g's block rows are g * H / 16 .. -- a column that survives in the
    last block row of gate 0 only must not appear in the first of gate 1."""
    H, A = 48, 5
    K = H + A
    W = np.zeros((3 * H, K), np.float32)
    W[H - 1, K - 1] = 1.0           # gate 0, last row, the last aux column
    W[H, 0] = 2.0                   # gate 1, first row
    W[2 * H + 16, H] = 3.0          # gate 2, second block row, the first aux column
    pk = _pack(W, 3)
    lists = _lists(pk, 3 * H)
    want = {H // 16 - 1: [K - 1], H // 16: [0], 2 * H // 16 + 1: [H]}
    for br, (cols, _, _, _) in enumerate(lists):
        assert list(cols) == want.get(br, []), (br, cols)
    assert np.array_equal(_scatter(pk, 3 * H, K), W)
    # a gate of 24 rows is no whole number of block rows: refused
    from wavernn_amd import _lib
    with pytest.raises(_lib.WrnnError, match='no multiple of 16'):
        _pack(np.zeros((72, 8), np.float32), 3)


def test_the_threshold_sits_at_41_percent(L):
    """A view is admitted when at most 41 % of the blocks survive, 100 * kept <= 41 * total (the threshold was one half until the kernel measured slower than
    wrnn_tile_kernel there: include/wavernn_amd.h).  Exactly 41 % is in, one block more is out; `block_mask` at 0.6 is in, at 0.5 out."""
    W = np.zeros((16, 100), np.float32)
    W[3, :41] = 1.0
    pk = _pack(W, 1)
    assert (pk['kept'], pk['total'], pk['admitted']) == (41, 100, True)
    W[9, 41] = 1.0
    pk = _pack(W, 1)
    assert (pk['kept'], pk['total'], pk['admitted']) == (42, 100, False)
    for gates, H, K in ((1, 64, 32), (3, 256, 288)):
        at60, at50 = _pack(_pruned(6, H, K, gates, 0.6), gates), _pack(_pruned(6, H, K, gates, 0.5), gates)
        assert at60['admitted'] and 0.40 <= at60['kept'] / at60['total'] <= 0.41
        assert not at50['admitted'] and 2 * at50['kept'] == at50['total']
    assert not _pack(np.ones((16, 4), np.float32), 1)['admitted'] and _pack(np.zeros((16, 4), np.float32), 1)['admitted']
