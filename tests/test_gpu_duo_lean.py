"""GPU tests (-m gpu) of the dense duo loop kernel's lean operand check: a lane of a polling stage looks at ONE word of each 16-byte
fragment instead of all four (csrc/wrnn_ring.h `frag_there`, csrc/wrnn_duo.hip header); `wrnn_options.tuning` bit 12 restores the full
check.  Every case runs `algo='duo'` with the default and with bit 12 -- the outputs must be the same bits -- and is compared with the
oracle at the suite's tolerances (MoL <= 1e-5, RAW class indices equal).  The shapes are the smallest that reach the launch boundaries the
check lives next to: slabs shorter than a hop and shorter than the re-arm distance, segments that run into the fold's zero pad, a ragged
group (fewer than 16 segments) at 1, 2 and 4 slots in flight on one cluster (4 slots: the operand loads are issued in front of the pending
back half), a `t_range` continuation.
"""
import numpy as np
import pytest
import torch

from helpers import MOL_TOL, oracle_loop_fn

pytestmark = pytest.mark.gpu

FULL_CHECK = 4096          # wrnn_options.tuning bit 12 (include/wavernn_amd.h)
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _case(mode, wseed, mseed, seed, frames, target, overlap, T=None):
    """Seeded inputs of a batched fold (B segments `target + overlap` apart) run for T steps -- by default the fold's own
    target + 2 overlap -- and the C oracle's output for them, computed once per session."""
    key = (mode, wseed, mseed, seed, frames, target, overlap, T)
    if key in _MEMO:
        return _MEMO[key]
    from oracle import wavernn_oracle as O
    from wavernn_amd.synthetic import random_state_dict, random_mel
    sd = random_state_dict(wseed, mode=mode)
    mel = random_mel(mseed, frames)
    m = O.pad_tensor(mel.T[None], 2, 'both')[0].T
    mels_up, aux_up = O.upsample_network(sd, m)
    aux = np.ascontiguousarray(aux_up[::275])
    L = mels_up.shape[0]
    B, stride = O.num_folds(L, target, overlap), target + overlap
    T = target + 2 * overlap if T is None else T
    noise = O.draw_noise(seed, mode, B, T)
    flat = np.concatenate([noise[0].reshape(T, B * 10), noise[1].reshape(T, B)], axis=1) if mode == 'MOL' else noise
    flat = np.ascontiguousarray(flat, np.float32)
    seg_pos = np.arange(B, dtype=np.int32) * np.int32(stride)
    seg_lim = np.full(B, L, dtype=np.int32)
    ref = oracle_loop_fn(sd, mode)(torch.from_numpy(mels_up), torch.from_numpy(aux), seg_pos, seg_lim, T, torch.from_numpy(flat), 275).numpy()
    _MEMO[key] = (sd, mels_up, aux, B, T, stride, L, flat, ref)
    return _MEMO[key]


def _engine(gpu, mode, case):
    from wavernn_amd.engine import LoopEngine
    sd, mels_up, aux, B, T, stride, L, flat, ref = case
    eng = LoopEngine(sd, mode, device=gpu)
    mu, au, nz = torch.from_numpy(mels_up).to(gpu), torch.from_numpy(aux).to(gpu), torch.from_numpy(flat).to(gpu)

    def run(**kw):
        out = eng.run(mu, au, B, T, stride, nz, 275, algo='duo', **kw).cpu().numpy()
        assert eng.last_loop_kernel() == 'wrnn_duo_kernel'
        return out
    return eng, (mu, au, nz), run


def test_fold_edge_slabs_and_full_check(gpu):
    """frames = 100, target = 220, overlap = 22 (the suite's small fold: segments 242 apart), run for 616 steps: every segment crosses two
    or three hop boundaries and the last two run past the end of the conditioning into the zero pad.  One launch, slabs of 97 steps
    (shorter than a hop) and slabs of 3 (shorter than the re-arm distance), each with the lean and with the full check: six outputs,
    the same bits, within 1e-5 of the oracle."""
    case = _case('MOL', 37, 137, 97, 100, 220, 22, T=616)
    sd, mels_up, aux, B, T, stride, L, flat, ref = case
    assert T >= 600 and (B - 1) * stride + T > L          # two hop boundaries; the zero pad is reached
    eng, _, run = _engine(gpu, 'MOL', case)
    whole = run()
    err = float(np.abs(whole - ref).max())
    print(f'B={B} T={T} max|hip - oracle| = {err:.3e}')
    assert err <= MOL_TOL
    for kw in (dict(tuning=FULL_CHECK), dict(slab_steps=97), dict(slab_steps=97, tuning=FULL_CHECK), dict(slab_steps=3),
               dict(slab_steps=3, tuning=FULL_CHECK)):
        assert np.array_equal(run(**kw), whole), kw


@pytest.mark.parametrize('depth', [1, 2, 4])
def test_ragged_groups_one_cluster(gpu, depth):
    """53 frames folded at target = 220, overlap = 22: 61 segments = four groups of 15, 15, 15 and 16 (three ragged ones) whose segments sit
    on different phases of their frames; one cluster with 1, 2 and 4 slots in flight (4, 2 and 1 rounds)."""
    case = _case('MOL', 13, 105, 81, 53, 220, 22)
    sd, mels_up, aux, B, T, stride, L, flat, ref = case
    assert B == 61
    eng, _, run = _engine(gpu, 'MOL', case)
    out = run(clusters=1, depth=depth)
    assert eng.last_loop_split()[2] == depth
    err = float(np.abs(out - ref).max())
    print(f'depth {depth}: max|hip - oracle| = {err:.3e}')
    assert err <= MOL_TOL
    assert np.array_equal(run(clusters=1, depth=depth, tuning=FULL_CHECK), out)


def test_continuation_into_existing_output(gpu):
    """The same ragged fold as [0, 100) and a `t_range = (100, T)` continuation into that output (4 slots on one cluster): the bits of the
    single call, with either check."""
    case = _case('MOL', 13, 105, 81, 53, 220, 22)
    sd, mels_up, aux, B, T, stride, L, flat, ref = case
    eng, (mu, au, nz), run = _engine(gpu, 'MOL', case)
    whole = run(clusters=1, depth=4)
    for tuning in (0, FULL_CHECK):
        kw = dict(algo='duo', clusters=1, depth=4, tuning=tuning)
        out = eng.run(mu, au, B, T, stride, nz[:100].contiguous(), 275, t_range=(0, 100), **kw)
        out = eng.run(mu, au, B, T, stride, nz[100:].contiguous(), 275, t_range=(100, T), out=out, **kw)
        assert np.array_equal(out.cpu().numpy(), whole), tuning


def test_raw_depth2_slabs(gpu):
    """9-bit RAW (the logits layer is polled by fragments too): two slots in flight, slabs of 97 steps; class indices equal to the
    oracle's, with either check."""
    case = _case('RAW', 11, 102, 78, 60, 220, 22)
    sd, mels_up, aux, B, T, stride, L, flat, ref = case
    eng, _, run = _engine(gpu, 'RAW', case)
    out = run(depth=2, slab_steps=97)
    assert np.array_equal(out, ref)
    assert np.array_equal(run(depth=2, slab_steps=97, tuning=FULL_CHECK), out)
