"""wrnn_sparse_kernel with TWO groups of <= 16 segments per cluster (wrnn_options.sparse_groups = 2; csrc/wrnn_sparse.hip, NS = 2) on the device: MoL,
GRU matrices and Linear layers 95 % block-pruned (NBP 48; 92 %: NBP 64), shipped dims and hop, 40 steps in slabs of 16 -- three launches, the state
of every slot handed over twice.  Checked against the C oracle on the masked weights (the MoL bound) and, bit for bit, against the same
call with one group per cluster: a segment's arithmetic does not depend on the cluster or slot it runs in.

A round of g groups puts groups 0-15 into the first slot of clusters 0-15 and groups 16-31 into the second, and the planner cuts n segments into
ceil(n / 16) groups: 17, 32 and 33 segments are 2, 2 and 3 groups -- two-group launches whose second slots are all EMPTY (nothing may wait for
them) --, 257 and 272 are 17 groups (ragged: 15 or 16 segments; full): the second slot live in cluster 0 alone beside sixteen first slots; the 512-segment
case fills all 32 slots.  So the live-second-slot cases are 257 and 272 (both NBP builds, a continued call included) and 512 (NBP 48)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, SLAB, STRIDE, HOP = 40, 16, 8, 275
MOL_TOL = 1e-5
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _pruned(sparsity):
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict
    return block_prune_state_dict(random_state_dict(52, mode='MOL'), sparsity, (16, 1), linear=True)[0]


def _case(gpu, sparsity, nmax):
    """Engine, conditioning (the up-sampled mel and the same mel one stage short), noise and the oracle's samples of `nmax` segments x T steps on
    block-pruned MoL weights -- computed once; a case of n <= nmax segments takes the first n (segments are independent of one another)."""
    key = (sparsity, nmax)
    if key not in _MEMO:
        from oracle import c_oracle as C
        from wavernn_amd.engine import LoopEngine, MelRows
        from wavernn_amd.pre import PreEngine
        from wavernn_amd.synthetic import random_mel
        sd = _pruned(sparsity)
        pre = PreEngine(sd, device=gpu)
        frames = -(-(nmax * STRIDE + T) // HOP) + 1
        mel = torch.from_numpy(random_mel(1500, frames)).to(gpu)
        mels_up, aux = pre.upsample(mel)
        rows = pre.upsample_rows(mel)[0]
        pos = np.arange(nmax)[:, None] * STRIDE + np.arange(T)[None]
        assert pos.max() < mels_up.shape[0] == frames * HOP and pre.scales[2] == 11
        g = torch.Generator().manual_seed(5)
        u1 = (torch.rand(T, nmax, 10, generator=g) * (1 - 2e-5) + 1e-5).numpy()
        u2 = (torch.rand(T, nmax, generator=g) * (1 - 2e-5) + 1e-5).numpy()
        ref = C.loop(sd, 'MOL', mels_up.cpu().numpy()[pos], aux.cpu().numpy()[pos // HOP], (u1, u2))
        mr = MelRows(rows, mels_up.shape[0], pre.scales[2], pre.last_taps, pre.pad * HOP)
        _MEMO[key] = (LoopEngine(sd, 'MOL', device=gpu), {'materialised': mels_up, 'in-loop': mr}, aux, (u1, u2), ref)
    return _MEMO[key]


def _noise(u, n, gpu, t0=0, t1=T):
    return torch.from_numpy(np.concatenate([u[0][t0:t1, :n].reshape(t1 - t0, n * 10), u[1][t0:t1, :n]], axis=1)).to(gpu).contiguous()


def _both_ways(gpu, sparsity, nmax, n, mel, nbp):
    eng, mels, aux, u, ref = _case(gpu, sparsity, nmax)
    assert (48 if nbp == 64 else 0) < eng.sparse_blocks <= nbp and 0 < eng.sparse_fc_blocks <= nbp
    outs = {}
    for groups in (2, 1):
        out = eng.run(mels[mel], aux, n, T, STRIDE, _noise(u, n, gpu), HOP, algo='sparse', slab_steps=SLAB, sparse_groups=groups)      # (check=True: wrnn_status is clean)
        info = eng.last_run_info()
        assert (info['kernel'], info['clusters'], info['depth'], info['slab_steps']) == ('wrnn_sparse_kernel', 16, groups, SLAB), info
        assert info['rounds'] == -(-(-(-n // 16)) // (16 * groups)) and info['launches'] == 3 * info['rounds'], info
        outs[groups] = out.cpu().numpy()
    err = np.abs(outs[2] - ref[:n]).max()
    print(f'{n} segments, NBP {nbp}, mel {mel}: max |two groups - oracle| = {err:.3e}, |one group - oracle| = {np.abs(outs[1] - ref[:n]).max():.3e}')
    assert err <= MOL_TOL, err
    bad = np.argwhere(outs[2] != outs[1])
    assert bad.size == 0, f'{len(bad)} samples differ from the one-group run, first at (segment, step) = {tuple(bad[0])}'


@pytest.mark.parametrize('mel', ['materialised', 'in-loop'])
@pytest.mark.parametrize('n', [17, 32, 33, 257, 272])
def test_two_groups_nbp48(gpu, n, mel):
    _both_ways(gpu, 0.95, 272, n, mel, 48)


@pytest.mark.parametrize('mel', ['materialised', 'in-loop'])
@pytest.mark.parametrize('n', [33, 257, 272])
def test_two_groups_nbp64(gpu, n, mel):
    """33: every second slot empty; 257 / 272: 17 groups -- cluster 0 runs a ragged / a full group in its SECOND slot of the NBP 64 build."""
    _both_ways(gpu, 0.92, 272, n, mel, 64)


@pytest.mark.parametrize('n,sparsity', [(33, 0.95), (257, 0.95), (272, 0.92)], ids=['33-empty-second-slots', '257-live-second-slot', '272-live-second-slot-nbp64'])
def test_two_groups_continue_a_call(gpu, n, sparsity):
    """Steps [0, 24) and then [24, 40) on one workspace: the samples of the single call (33 segments: the issue's case; 257 / 272: a live second slot's
    state crosses the call boundary too)."""
    eng, mels, aux, u, ref = _case(gpu, sparsity, 272)
    kw = dict(algo='sparse', slab_steps=SLAB, sparse_groups=2)
    whole = eng.run(mels['materialised'], aux, n, T, STRIDE, _noise(u, n, gpu), HOP, **kw).cpu().numpy()
    out = None
    for t0, t1 in ((0, 24), (24, T)):
        out = eng.run(mels['materialised'], aux, n, T, STRIDE, _noise(u, n, gpu, t0, t1), HOP, t_range=(t0, t1), out=out, **kw)
        assert eng.last_run_info()['depth'] == 2
    assert np.array_equal(out.cpu().numpy(), whole)
    assert np.abs(whole - ref[:n]).max() <= MOL_TOL


def test_two_groups_fill_all_32_slots(gpu):
    """512 segments x 1,700 steps (one slab boundary at the default slab length): one round of 32 groups == two rounds of 16, bit for bit."""
    from wavernn_amd.engine import LoopEngine
    n, steps = 512, 1700
    eng = LoopEngine(_pruned(0.95), 'MOL', device=gpu)
    rs = np.random.RandomState(3)
    L = (n * STRIDE + steps + HOP - 1) // HOP * HOP
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, 80)).astype(np.float32)).to(gpu)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 128)).astype(np.float32)).to(gpu)
    noise = (torch.rand(steps, 11 * n, generator=torch.Generator().manual_seed(7)) * (1 - 2e-5) + 1e-5).to(gpu)
    outs = {}
    for groups in (2, 1):
        outs[groups] = eng.run(mels_up, aux, n, steps, STRIDE, noise, HOP, algo='sparse', sparse_groups=groups).cpu().numpy()
        info = eng.last_run_info()
        assert (info['kernel'], info['depth'], info['rounds'], info['launches']) == ('wrnn_sparse_kernel', groups, 3 - groups, 2 * (3 - groups)), info
    assert np.isfinite(outs[2]).all() and np.array_equal(outs[2], outs[1])


def test_two_groups_through_the_model(gpu, tmp_path):
    """`model.sparse_groups = 2`: generate_corpus() on two short utterances that fold to more than 16 segments, and generate(), give the waveforms of
    `sparse_groups = None`, and the run info says two groups per cluster."""
    from wavernn_amd.batch import generate_corpus
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel, SHIPPED
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in _pruned(0.95).items()}, strict=True)
    model = model.to(gpu)
    mels = [torch.from_numpy(random_mel(1600 + k, f)).unsqueeze(0) for k, f in enumerate((24, 22))]
    got = {}
    for groups in (None, 2):
        model.sparse_groups = groups
        waves = generate_corpus(model, mels, 550, 55, True, [71, 72])
        info = model._loop_engine().last_run_info()
        assert info['kernel'] == 'wrnn_sparse_kernel' and info['depth'] == (groups or 1), info
        torch.manual_seed(81)
        one = model.generate(mels[0], tmp_path / f'g{groups}.wav', True, 550, 55, False)
        assert model.last_loop_kernel == 'wrnn_sparse_kernel' and model._loop_engine().last_run_info()['depth'] == (groups or 1)
        got[groups] = [np.asarray(w, np.float64) for w in waves] + [np.asarray(one, np.float64)]
    from wavernn_amd.fold import fold_geometry
    assert sum(fold_geometry(f * HOP, 550, 55)[0] for f in (24, 22)) > 16
    for a, b in zip(got[None], got[2]):
        assert a.shape == b.shape and a.size > 0 and np.array_equal(a, b)
    # a dense model ignores the attribute: no error, another kernel
    dense = WaveRNN(**SHIPPED, mode='MOL').to(gpu)
    dense.sparse_groups = 2
    dense.generate(mels[0], tmp_path / 'dense.wav', True, 550, 55, False)
    assert dense.last_loop_kernel != 'wrnn_sparse_kernel'
