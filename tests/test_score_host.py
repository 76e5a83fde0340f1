"""The scoring path without a GPU: `wrnn_nll_host` against the reference's own loss functions (tests/golden/score_loss_cases.npz, written by
scripts/make_golden_score.py), its sums and masks, the argument checks of both entry points, the target preparation against the reference's
preprocessing (tests/golden/score_forward_3utt.npz) and the host logic of `score_corpus` (segment table, chunker)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

HOP = 275
KINDS = [('mol', 'MOL'), ('raw512', 'RAW'), ('raw256', 'RAW')]
_MEMO = {}


def loss_case(kind):
    """(logits [T][n][C], labels [n][T], the fixture) of a loss case -- the seeded inputs rebuilt, checked against the stored sample of them."""
    if kind not in _MEMO:
        from wavernn_amd.synthetic import score_loss_inputs
        g = np.load(os.path.join(GOLDEN, 'score_loss_cases.npz'))
        lg, lab = score_loss_inputs(kind, int(g['seed']))
        assert np.array_equal(lg.reshape(-1)[::97], g[kind + '_logits_strided']), 'the rebuilt inputs are not the ones the reference scored'
        assert np.array_equal(lab, g[kind + '_labels'].astype(np.int64))
        _MEMO[kind] = (lg, lab, g)
    return _MEMO[kind]


def check_against_reference(kind, ours, what):
    """max |ours - ref64| <= 2 E_ref, E_ref = max |ref32 - ref64|: the reference's own float32 distance from exact arithmetic; the factor 2 allows for
    another exp / log and for a mixture term on the other side of `cdf_delta > 1e-5`, where the two branches agree to that order."""
    g = loss_case(kind)[2]
    ref32, ref64 = g[kind + '_ref32'], g[kind + '_ref64']
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(ours.astype(np.float64) - ref64).max())
    print(f'{what} {kind}: E_ref = {e_ref:.3e}, max |ours - ref64| = {err:.3e}')
    assert ours.shape == ref64.shape and np.isfinite(ours).all()
    assert e_ref > 0 and err <= 2 * e_ref, (kind, err, e_ref)


@pytest.mark.parametrize('kind,mode', KINDS)
def test_host_loss_matches_the_reference(kind, mode):
    from wavernn_amd import _lib
    lg, lab, g = loss_case(kind)
    nll, total = _lib.nll_host(mode, lg, g[kind + '_target'])
    check_against_reference(kind, nll, 'wrnn_nll_host')
    if mode == 'RAW':       # the class recovered from the target value is the stored label, for every element: -log p is then read off that class
        C = lg.shape[2]
        x = g[kind + '_target']
        assert np.array_equal(np.rint((x.astype(np.float32) + np.float32(1)) * np.float32(C - 1) * np.float32(0.5)).astype(np.int64), lab)
        m = lg.max(axis=2, keepdims=True).astype(np.float64)
        lse = m[..., 0] + np.log(np.exp(lg.astype(np.float64) - m).sum(axis=2))                 # [T][n]
        at_label = lse - np.take_along_axis(lg.astype(np.float64), lab.T[..., None], axis=2)[..., 0]
        off_by_one = lse - np.take_along_axis(lg.astype(np.float64), ((lab.T + 1) % C)[..., None], axis=2)[..., 0]
        assert np.abs(nll.T - at_label).max() < 1e-4 < np.abs(nll.T - off_by_one).max()


def test_mol_branches_are_all_exercised():
    """The MOL set reaches every selection of distribution.py:69-77 (the shares scripts/make_golden_score.py asserts, restated in float64)."""
    lg, lab, g = loss_case('mol')
    y = g['mol_target'].astype(np.float64).T[..., None]
    assert g['mol_target'].min() == -1.0 and g['mol_target'].max() == 1.0
    assert np.array_equal(g['mol_target'], np.float32(2) * lab.astype(np.float32) / np.float32(65535) - np.float32(1))
    inv = np.exp(-lg[..., 20:].astype(np.float64))
    cy = y - lg[..., 10:20]
    delta = 1 / (1 + np.exp(-inv * (cy + 1 / 65535))) - 1 / (1 + np.exp(-inv * (cy - 1 / 65535)))
    assert (y < -0.999).mean() >= 0.02 and (y > 0.999).mean() >= 0.02 and 0.2 <= (delta > 1e-5).mean() <= 0.9


@pytest.mark.parametrize('kind,mode', KINDS[:2])
def test_sums_and_masks(kind, mode):
    from wavernn_amd import _lib
    lg, _, g = loss_case(kind)
    x = g[kind + '_target']
    T, n, _ = lg.shape
    nll, total = _lib.nll_host(mode, lg, x)
    np.testing.assert_allclose(total, nll.astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)
    _, total_only = _lib.nll_host(mode, lg, x, per_step=False)               # nll = NULL: the same sums
    assert np.array_equal(total_only, total)
    lens = np.array([0, 1, T - 1, T, 17, 63, 64, 65][:n] + [T // 2] * max(0, n - 8), np.int32)[:n]
    lens = np.minimum(lens, T)
    masked, msum = _lib.nll_host(mode, lg, x, seg_len=lens)
    for b in range(n):
        assert np.array_equal(masked[b, :lens[b]], nll[b, :lens[b]]) and not masked[b, lens[b]:].any()
    np.testing.assert_allclose(msum, masked.astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)
    assert msum[0] == 0.0 and lens[0] == 0
    # steps past seg_len are not read: garbage there changes nothing
    dirty = lg.copy()
    for b in range(n):
        dirty[lens[b]:, b] = np.nan
    again, asum = _lib.nll_host(mode, dirty, x, seg_len=lens)
    assert np.array_equal(again, masked) and np.array_equal(asum, msum)
    # a segment alone gives the bits it gives among the others
    alone, alsum = _lib.nll_host(mode, lg[:, 3:4], x[3:4])
    assert np.array_equal(alone[0], nll[3]) and alsum[0] == total[3]


def _call(**kw):
    from wavernn_amd import _lib
    T, n, C = 3, 2, kw.pop('C', 30)
    bufs = dict(logits=np.zeros((T, n, C), np.float32), target=np.zeros((n, T), np.float32), sum=np.zeros(n, np.float64))
    c = _lib.NllCall(mode=_lib.MODE_MOL, n_classes=C, n_segments=n, T=T, **{k: v.ctypes.data for k, v in bufs.items()})
    for k, v in kw.items():
        setattr(c, k, v)
    return c, bufs


BAD_CALLS = [
    (dict(struct_bytes=8), 'struct_bytes is 8'),
    (dict(logits=None), 'NULL logits'),
    (dict(target=None), 'NULL target'),
    (dict(sum=None), 'NULL sum'),
    (dict(mode=7), 'unknown mode 7'),
    (dict(n_classes=29), 'MOL scores 30 outputs per step (10 mixtures), not 29'),
    (dict(mode=0, n_classes=1), 'RAW scores 2..2048 classes, not 1'),
    (dict(mode=0, n_classes=2049), 'RAW scores 2..2048 classes, not 2049'),
    (dict(n_segments=0), 'bad shape: 0 segments, 3 steps'),
    (dict(T=0), 'bad shape: 2 segments, 0 steps'),
]


@pytest.mark.parametrize('entry', ['wrnn_nll', 'wrnn_nll_host'])
@pytest.mark.parametrize('fields,message', BAD_CALLS, ids=[m for _, m in BAD_CALLS])
def test_bad_arguments_are_refused_before_anything_runs(entry, fields, message):
    from wavernn_amd import _lib
    L = _lib.lib()
    c, bufs = _call(**fields)
    bufs['sum'][:] = 123.0
    rc = L.wrnn_nll(0, ctypes.byref(c)) if entry == 'wrnn_nll' else L.wrnn_nll_host(ctypes.byref(c))
    assert rc == _lib.ERR_ARG, rc
    assert message in L.wrnn_last_error().decode(), L.wrnn_last_error()
    assert (bufs['sum'] == 123.0).all()
    assert (L.wrnn_nll(0, None) if entry == 'wrnn_nll' else L.wrnn_nll_host(None)) == _lib.ERR_ARG


def test_device_entry_point_needs_a_device():
    """Valid arguments: the host entry point computes, the device one says WRNN_ERR_NO_DEVICE where there is none (never a host fallback)."""
    from wavernn_amd import _lib
    L = _lib.lib()
    c, bufs = _call()
    bufs['sum'][:] = 123.0
    assert L.wrnn_nll_host(ctypes.byref(c)) == _lib.WRNN_OK and np.isfinite(bufs['sum']).all() and (bufs['sum'] != 123.0).all()
    if not torch.cuda.is_available():       # (host pointers: only where the call cannot launch)
        bufs['sum'][:] = 123.0
        assert L.wrnn_nll(0, ctypes.byref(c)) == _lib.ERR_NO_DEVICE
        assert b'no HIP device' in L.wrnn_last_error() and (bufs['sum'] == 123.0).all()


def test_target_preparation_matches_the_reference():
    """Labels (16-bit, 9-bit linear, 9-bit mu-law) and the values fed / scored equal what the reference's preprocessing and data loader made of the
    same waveforms."""
    from wavernn_amd.score import prepare_targets
    g = np.load(os.path.join(GOLDEN, 'score_forward_3utt.npz'))
    for u, frames in enumerate(g['frames']):
        w = g[f'wav{u}']
        assert w.dtype == np.float32 and w.shape == (frames * HOP,) and np.abs(w).max() == 1.0
        lab, val = prepare_targets(w, 'MOL')
        assert np.array_equal(lab, g[f'labels16_{u}'].astype(np.int64)) and np.array_equal(val, g[f'mol_target{u}']) and val.dtype == np.float32
        lab, val = prepare_targets(w, 'RAW', bits=9, mu_law=True)
        assert np.array_equal(lab, g[f'labels9mu_{u}'].astype(np.int64)) and np.array_equal(val, g[f'raw_target{u}'])
        lab, _ = prepare_targets(w, 'RAW', bits=9, mu_law=False)
        assert np.array_equal(lab, g[f'labels9_{u}'].astype(np.int64))
        lab2, val2 = prepare_targets(g[f'labels9mu_{u}'], 'RAW', bits=9)                  # an integer array is taken as labels
        assert np.array_equal(lab2, g[f'labels9mu_{u}'].astype(np.int64)) and np.array_equal(val2, g[f'raw_target{u}'])
    with pytest.raises(ValueError):
        prepare_targets(np.array([0.0, 1.5], np.float32), 'MOL')
    with pytest.raises(ValueError):
        prepare_targets(np.array([0, 512]), 'RAW', bits=9)


def test_fixture_loss_is_the_loss_of_the_fixture_logits():
    """Ties the two fixtures together on the CPU: `wrnn_nll_host` on the stored rows of the reference's teacher-forced logits gives the reference's
    per-step NLL at those rows, within the fixture's own float32 scale (the loss-case bound, 2 E_ref of the MOL / RAW-512 sets)."""
    from wavernn_amd import _lib
    g = np.load(os.path.join(GOLDEN, 'score_forward_3utt.npz'))
    for mode, kind in (('MOL', 'mol'), ('RAW', 'raw512')):
        lc = loss_case(kind)[2]
        bound = 2 * float(np.abs(lc[kind + '_ref32'].astype(np.float64) - lc[kind + '_ref64']).max())
        k = mode.lower()
        for u in range(3):
            rows = g[f'{k}_logits{u}']
            nll, _ = _lib.nll_host(mode, rows[:, None, :], g[f'{k}_target{u}'][::97][None])
            err = float(np.abs(nll[0] - g[f'{k}_nll{u}'][::97]).max())
            print(f'{mode} utterance {u}: max |ours - ref| on {rows.shape[0]} rows = {err:.3e} (bound {bound:.3e})')
            assert err <= bound


def test_scoring_segment_table():
    from wavernn_amd.score import segment_table
    pos, lim = segment_table([9, 17, 24], [9 * HOP, 17 * HOP - 100, 1], HOP)
    assert pos.dtype == np.int32 and lim.dtype == np.int32
    assert pos.tolist() == [0, 9 * HOP, 26 * HOP] and lim.tolist() == [9 * HOP, 26 * HOP - 100, 26 * HOP + 1]
    assert (pos % HOP == 0).all()               # every utterance starts on a frame boundary
    with pytest.raises(ValueError):
        segment_table([9], [9 * HOP + 1], HOP)
    with pytest.raises(ValueError):
        segment_table([9], [0], HOP)
    with pytest.raises(ValueError, match='int32'):
        segment_table([4000000, 4000000], [5, 5], HOP)


def test_chunker_respects_the_budget_and_the_callers_order():
    from wavernn_amd.score import chunk_by_bytes
    rs = np.random.RandomState(5)
    steps = rs.randint(1, 5000, size=37).tolist() + [5000, 5000, 1]
    C = 30
    for budget in (5000 * C * 4, 3 * 5000 * C * 4 + 7, 10 ** 9):
        chunks = chunk_by_bytes(steps, C, budget)
        assert all(len(c) > 0 for c in chunks)
        assert sorted(u for c in chunks for u in c) == list(range(len(steps)))
        for c in chunks:
            assert max(steps[u] for u in c) * len(c) * C * 4 <= budget
        flat = [u for c in chunks for u in c]
        assert [steps[u] for u in flat] == sorted(steps)          # sorted by length: T stays tight
        out = [None] * len(steps)                                 # results scattered back by index restore the caller's order
        for c in chunks:
            for u in c:
                out[u] = steps[u]
        assert out == steps
    assert len(chunk_by_bytes(steps, C, 10 ** 9)) == 1 and len(chunk_by_bytes(steps, C, 5000 * C * 4)) > 3
    with pytest.raises(ValueError, match=str(5000 * C * 4)):
        chunk_by_bytes(steps, C, 5000 * C * 4 - 1)


def test_score_needs_a_hip_device():
    """No CPU path: a model on the host refuses to score."""
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import SHIPPED
    model = WaveRNN(**SHIPPED, mode='MOL')
    assert model.score_logits_bytes == 8 << 30
    with pytest.raises(RuntimeError, match='HIP device'):
        model.score(torch.zeros(1, 80, 3), np.zeros(3 * HOP, np.float32))
