"""wrnn_slab_prep_kernel (csrc/wrnn_cond.hip): the one launch that prepares a conditioning slab of the slabbed loop kernels -- derived MoL noise, the
slab's aux tables, the placement words cleared -- against the three calls it replaces (wrnn_options.tuning bit 13), sample for sample.

One 60-frame utterance folded at target 550 / overlap 55 (T = 660, 28 segments = two groups), shipped dims: MoL and 9-bit RAW on wrnn_duo_kernel at two
groups per cluster with slabs of 97 steps (7 slabs, the last one short; 3 table rows per segment) and of 3 steps (220 slabs, 2 rows); MoL on
wrnn_chain_kernel and, with a 95 % block-pruned pack, on wrnn_sparse_kernel; and one call continued across a slab boundary (t_range)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, TARGET, OVERLAP, HOP = 60, 550, 55, 275
T, STRIDE = TARGET + 2 * OVERLAP, TARGET + OVERLAP
SPLIT = 8192              # wrnn_options.tuning bit 13
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    return torch.device('cuda', 0)


def _case(gpu, mode, pruned):
    """Engine, conditioning and noise of the case: made once per (mode, pack)."""
    key = (mode, pruned)
    if key not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        from wavernn_amd.fold import fold_geometry
        from wavernn_amd.pre import PreEngine
        from wavernn_amd.rng import draw_steps
        from wavernn_amd.synthetic import random_mel, random_state_dict
        sd = random_state_dict(41, mode=mode)
        if pruned:
            from wavernn_amd.prune import block_prune_state_dict
            sd = block_prune_state_dict(sd, 0.95, (16, 1), linear=True)[0]
        mels_up, aux = PreEngine(sd, device=gpu).upsample(torch.from_numpy(random_mel(1800, FRAMES)).to(gpu))
        B = fold_geometry(FRAMES * HOP, TARGET, OVERLAP)[0]
        assert B == 28
        eng = LoopEngine(sd, mode, device=gpu)
        torch.manual_seed(97)
        noise = draw_steps(mode, B, T, eng.n_classes, gpu, 'device')
        _MEMO[key] = (eng, mels_up, aux, B, noise)
    return _MEMO[key]


def _both(gpu, mode, algo, slab, pruned=False, **kw):
    eng, mels_up, aux, B, noise = _case(gpu, mode, pruned)
    outs = {}
    for tuning in (0, SPLIT):
        out = eng.run(mels_up, aux, B, T, STRIDE, noise, HOP, algo=algo, slab_steps=slab, tuning=tuning, **kw)       # (check=True: wrnn_status is clean)
        info = eng.last_run_info()
        assert info['kernel'] == f'wrnn_{algo}_kernel' and info['slab_steps'] == slab and info['launches'] == -(-T // slab) * info['rounds'], info
        outs[tuning] = out.cpu().numpy()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() <= 1.0 and outs[0].std() > 0
    bad = np.argwhere(outs[0] != outs[SPLIT])
    assert bad.size == 0, f'{len(bad)} samples differ from the three-call path, first at (segment, step) = {tuple(bad[0])}'
    return outs[0]


@pytest.mark.parametrize('slab', [97, 3])
@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_duo(gpu, mode, slab):
    _both(gpu, mode, 'duo', slab, depth=2)
    assert _case(gpu, mode, False)[0].last_run_info()['depth'] == 2


def test_chain_mol(gpu):
    _both(gpu, 'MOL', 'chain', 97)


def test_sparse_mol_95(gpu):
    eng = _case(gpu, 'MOL', True)[0]
    assert 0 < eng.sparse_blocks <= 48
    _both(gpu, 'MOL', 'sparse', 97, pruned=True)


@pytest.mark.parametrize('tuning', [0, SPLIT], ids=['fused', 'three-calls'])
def test_continuation_across_a_slab_boundary(gpu, tuning):
    """Steps [0, 300) and then [300, 660) in slabs of 97: the second call starts inside what would be the whole call's fourth slab; its first slab has
    its own table origin and noise rows.  The samples of the single fused call."""
    eng, mels_up, aux, B, noise = _case(gpu, 'MOL', False)
    whole = _both(gpu, 'MOL', 'duo', 97, depth=2)
    out = None
    for t0, t1 in ((0, 300), (300, T)):
        out = eng.run(mels_up, aux, B, T, STRIDE, noise[t0:t1].contiguous(), HOP, algo='duo', depth=2, slab_steps=97, tuning=tuning, t_range=(t0, t1), out=out)
    assert np.array_equal(out.cpu().numpy(), whole)
