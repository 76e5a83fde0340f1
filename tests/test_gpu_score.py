"""The scoring path on the GPU: `wrnn_nll` against the reference's loss functions, `score_corpus` / `score` against the reference's teacher-forced
forward and loss (tests/golden/score_forward_3utt.npz), the same score from every loop kernel, masks, the pruning sweep, and generation untouched.

The end-to-end bound is the fixture's `nll_sensitivity`: the largest per-step change of the reference's OWN loss when its logits move by the project's
teacher-forced logits tolerance (1e-4, tests/test_gpu_parity.py) -- the kernels may be that far off in the logits, so the loss may move by that much."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, MOL_TOL, load_case
from test_score_host import HOP, KINDS, check_against_reference, loss_case

pytestmark = pytest.mark.gpu
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def fixture():
    if 'fix' not in _MEMO:
        _MEMO['fix'] = np.load(os.path.join(GOLDEN, 'score_forward_3utt.npz'))
    return _MEMO['fix']


def bound_of(mode):
    """per-step bound: the reference's own sensitivity to 1e-4 in the logits; RAW also <= 2e-4 (cross-entropy moves by at most twice the largest
    logit change)"""
    s = float(fixture()[f'{mode.lower()}_nll_sensitivity'])
    assert s > 0
    return min(s, 2e-4) if mode == 'RAW' else s


def shipped_model(gpu, mode, sd=None, key=None):
    """The fixture's model (weights `random_state_dict(12, 'MOL')` / `(11, 'RAW')`) on the device; memoised, never written to."""
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, SHIPPED
    key = ('model', mode, key)
    if key not in _MEMO:
        g = fixture()
        sd = random_state_dict(int(g[f'wseed_{mode.lower()}']), mode=mode) if sd is None else sd
        model = WaveRNN(**SHIPPED, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        _MEMO[key] = model.to(gpu)
    return _MEMO[key]


def fixture_utterances():
    from wavernn_amd.synthetic import random_mel
    g = fixture()
    mels = [torch.from_numpy(random_mel(int(s), int(n))).unsqueeze(0) for s, n in zip(g['mel_seeds'], g['frames'])]
    return mels, [g[f'wav{u}'] for u in range(len(mels))]


def short_wave(n, seed=9):
    rs = np.random.RandomState(seed)
    return np.clip(0.5 * np.sin(np.arange(n) * 0.05) + 0.02 * rs.standard_normal(n), -1, 1).astype(np.float32)


# ---- the loss kernel --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,mode', KINDS)
def test_device_loss(gpu, kind, mode):
    """`wrnn_nll` on the inputs the reference scored: within 2 E_ref of the reference's float64 result; two launches give the same bits; a segment
    scored alone gives the bits it gives among 16; steps past seg_len are 0, are not read and do not count."""
    from wavernn_amd import _lib
    from wavernn_amd.score import nll_on_device
    lg, _, g = loss_case(kind)
    T, n, C = lg.shape
    L = _lib.lib()
    logits, x = torch.from_numpy(lg).to(gpu), torch.from_numpy(g[kind + '_target']).to(gpu)
    full = torch.full((n,), T, dtype=torch.int32, device=gpu)

    def run(lo, tg, lens, per_step=True):
        nll, total = nll_on_device(L, 0, mode, lo, tg, lens, per_step)
        torch.cuda.synchronize()
        return (nll.cpu().numpy() if per_step else None), total.cpu().numpy()
    nll, total = run(logits, x, full)
    check_against_reference(kind, nll, 'wrnn_nll')
    np.testing.assert_allclose(total, nll.astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)
    nll2, total2 = run(logits, x, full)
    assert np.array_equal(nll2, nll) and np.array_equal(total2, total)
    assert np.array_equal(run(logits, x, full, per_step=False)[1], total)            # nll = NULL: the same sums
    alone, alsum = run(logits[:, 5:6].contiguous(), x[5:6].contiguous(), full[5:6])
    assert np.array_equal(alone[0], nll[5]) and alsum[0] == total[5]
    lens = np.minimum(np.array([0, 1, T - 1, T, 17, 63, 64, 65] + [T // 2] * (n - 8), np.int32), T)
    dirty = lg.copy()
    for b in range(n):
        dirty[lens[b]:, b] = np.nan
    masked, msum = run(torch.from_numpy(dirty).to(gpu), x, torch.from_numpy(lens).to(gpu))
    for b in range(n):
        assert np.array_equal(masked[b, :lens[b]], nll[b, :lens[b]]) and not masked[b, lens[b]:].any()
    np.testing.assert_allclose(msum, masked.astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)
    assert msum[0] == 0.0


def test_device_loss_on_an_odd_class_count(gpu):
    """RAW with a class count that is no multiple of 4 (the scalar row path) and rows that are not 16-byte aligned: against float64 numpy."""
    from wavernn_amd import _lib
    from wavernn_amd.score import nll_on_device
    rs = np.random.RandomState(3)
    T, n, C = 37, 3, 1023
    lg = rs.normal(0, 4, size=(T, n, C)).astype(np.float32)
    lab = rs.randint(0, C, size=(n, T))
    lab[0, :2] = 0, C - 1
    x = (np.float32(2) * lab.astype(np.float32) / np.float32(C - 1) - np.float32(1)).astype(np.float32)
    nll, total = nll_on_device(_lib.lib(), 0, 'RAW', torch.from_numpy(lg).to(gpu), torch.from_numpy(x).to(gpu),
                               torch.full((n,), T, dtype=torch.int32, device=gpu), True)
    torch.cuda.synchronize()
    m = lg.max(axis=2, keepdims=True).astype(np.float64)
    ref = (m[..., 0] + np.log(np.exp(lg - m).sum(axis=2)) - np.take_along_axis(lg.astype(np.float64), lab.T[..., None], axis=2)[..., 0]).T
    host = _lib.nll_host('RAW', lg, x)[0]
    e_host = float(np.abs(host - ref).max())
    err = float(np.abs(nll.cpu().numpy() - ref).max())
    print(f'C = {C}: device {err:.3e}, host {e_host:.3e} from float64')
    assert err <= 2 * max(e_host, float(np.spacing(np.float32(ref.max()))))       # the host's float32 distance from exact arithmetic, at least one ulp
    np.testing.assert_allclose(total.cpu().numpy(), nll.cpu().numpy().astype(np.float64).sum(axis=1), rtol=1e-12, atol=0)


# ---- end to end against the reference ---------------------------------------------------------------------------------------------------------------
def corpus_scores(gpu, mode):
    """`score_corpus` on the three fixture utterances in ONE call (ragged, T = 6,600, `auto`); memoised and left unchanged."""
    if ('corpus', mode) not in _MEMO:
        from wavernn_amd.batch import score_corpus
        model = shipped_model(gpu, mode)
        mels, wavs = fixture_utterances()
        res = score_corpus(model, mels, wavs, mu_law=True, per_step=True)
        _MEMO[('corpus', mode)] = (res, model.last_loop_kernel)
    return _MEMO[('corpus', mode)]


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_score_corpus_matches_the_reference(gpu, mode):
    g, k, bound = fixture(), mode.lower(), bound_of(mode)
    res, kernel = corpus_scores(gpu, mode)
    assert kernel == 'wrnn_chain_kernel', kernel            # what `auto` picks for three segments of a dense model
    for u, r in enumerate(res):
        ref = g[f'{k}_nll{u}']
        assert r['steps'] == ref.shape[0] == int(g['frames'][u]) * HOP and r['per_step'].shape == ref.shape and r['per_step'].dtype == np.float32
        err = float(np.abs(r['per_step'] - ref).max())
        print(f'{mode} utterance {u} ({kernel}): max per-step |ours - ref| = {err:.3e} (bound {bound:.3e}); mean {r["nll_mean"]:.6f} vs {float(g[k + "_nll_mean"][u]):.6f}')
        assert err <= bound
        assert abs(r['nll_mean'] - float(g[k + '_nll_mean'][u])) <= bound
        assert r['nll_sum'] == pytest.approx(r['per_step'].astype(np.float64).sum(), rel=1e-12)
        assert r['bits_per_sample'] == pytest.approx(r['nll_mean'] / np.log(2), rel=1e-12)


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_score_of_one_utterance(gpu, mode):
    """`WaveRNN.score` on utterance 0 alone (B = 1, T = 2,475): the reference's per-step values, and those of the corpus call."""
    g, k, bound = fixture(), mode.lower(), bound_of(mode)
    model = shipped_model(gpu, mode)
    mels, wavs = fixture_utterances()
    r = model.score(mels[0], wavs[0], mu_law=True, per_step=True)
    assert r['steps'] == 9 * HOP
    assert float(np.abs(r['per_step'] - g[f'{k}_nll0']).max()) <= bound
    assert float(np.abs(r['per_step'] - corpus_scores(gpu, mode)[0][0]['per_step']).max()) <= bound
    assert 'per_step' not in model.score(mels[0], wavs[0], mu_law=True)
    if mode == 'RAW':            # labels in, the same score
        r2 = model.score(mels[0], g['labels9mu_0'], per_step=True)
        assert np.array_equal(r2['per_step'], r['per_step'])


def test_chunked_corpus_gives_the_same_scores(gpu):
    """A logits budget that holds one of the three utterances at a time: three chunks, the results in the caller's order."""
    from wavernn_amd.batch import score_corpus
    model = shipped_model(gpu, 'MOL')
    mels, wavs = fixture_utterances()
    order = [2, 0, 1]
    model.score_logits_bytes = 24 * HOP * 30 * 4
    try:
        res = score_corpus(model, [mels[u] for u in order], [wavs[u] for u in order], per_step=True)
        with pytest.raises(ValueError, match=str(24 * HOP * 30 * 4)):
            model.score_logits_bytes -= 1
            score_corpus(model, mels, wavs)
    finally:
        model.score_logits_bytes = 8 << 30
    whole = corpus_scores(gpu, 'MOL')[0]
    for r, u in zip(res, order):
        assert r['steps'] == whole[u]['steps'] and float(np.abs(r['per_step'] - whole[u]['per_step']).max()) <= bound_of('MOL')


# ---- every kernel gives the same score --------------------------------------------------------------------------------------------------------------
def test_every_dense_kernel_gives_the_same_score(gpu):
    """129 copies of a 3-frame utterance (825 steps) through `auto` -- more than 128 segments: the dense throughput kernel --, 3 through `chain` and
    `stream`: every per-step value within the bound of the others."""
    from wavernn_amd.batch import score_corpus
    from wavernn_amd.synthetic import random_mel
    model, bound = shipped_model(gpu, 'MOL'), bound_of('MOL')
    mel, wav = torch.from_numpy(random_mel(140, 3)).unsqueeze(0), short_wave(3 * HOP)
    res = score_corpus(model, [mel] * 129, [wav] * 129, per_step=True)
    assert model.last_loop_kernel == 'wrnn_duo_kernel', model.last_loop_kernel
    base = res[0]['per_step']
    assert base.shape == (825,) and np.isfinite(base).all()
    assert max(float(np.abs(r['per_step'] - base).max()) for r in res) <= bound
    for algo, kernel in (('chain', 'wrnn_chain_kernel'), ('stream', 'wrnn_stream_kernel')):
        few = score_corpus(model, [mel] * 3, [wav] * 3, per_step=True, algo=algo)
        assert model.last_loop_kernel == kernel, (algo, model.last_loop_kernel)
        err = max(float(np.abs(r['per_step'] - base).max()) for r in few)
        print(f'{algo}: max per-step |{kernel} - wrnn_duo_kernel| = {err:.3e} (bound {bound:.3e})')
        assert err <= bound


def oracle_forced_logits(sd, mels, aux, x_fed):
    """`oracle.wavernn_oracle.loop` (fatchord_version.py:203-223) teacher-forced: its cells and its float32 products, with x_fed[t] fed back after
    step t (step 0 reads 0).  mels [1, T, M], aux [1, T, 4 A] -> logits [T, 1, C]."""
    from oracle import wavernn_oracle as O
    F32 = np.float32
    g = lambda k: np.ascontiguousarray(sd[k], dtype=F32)
    T, d = mels.shape[1], aux.shape[2] // 4
    H = g('rnn1.weight_hh_l0').shape[1]
    h1, h2, x = np.zeros((1, H), F32), np.zeros((1, H), F32), np.zeros((1, 1), F32)
    out = []
    for i in range(T):
        a1, a2, a3, a4 = (aux[:, i, d * k:d * (k + 1)] for k in range(4))
        xx = (np.concatenate([x, mels[:, i, :], a1], axis=1) @ g('I.weight').T + g('I.bias')).astype(F32)
        h1 = O.gru_cell(xx, h1, g('rnn1.weight_ih_l0'), g('rnn1.weight_hh_l0'), g('rnn1.bias_ih_l0'), g('rnn1.bias_hh_l0'))
        xx = xx + h1
        h2 = O.gru_cell(np.concatenate([xx, a2], axis=1), h2, g('rnn2.weight_ih_l0'), g('rnn2.weight_hh_l0'), g('rnn2.bias_ih_l0'), g('rnn2.bias_hh_l0'))
        xx = xx + h2
        xx = np.maximum(np.concatenate([xx, a3], axis=1) @ g('fc1.weight').T + g('fc1.bias'), 0).astype(F32)
        xx = np.maximum(np.concatenate([xx, a4], axis=1) @ g('fc2.weight').T + g('fc2.bias'), 0).astype(F32)
        out.append((xx @ g('fc3.weight').T + g('fc3.bias')).astype(F32))
        x = x_fed[None, i:i + 1].astype(F32)
    return np.stack(out)


def test_other_model_dims_score_on_the_fallback_kernels(gpu):
    """A 256 / 256 MoL model (not the shipped dims): `auto` (wrnn_generic_kernel) and `algo='tile'` (wrnn_tile_kernel) give the score of the
    oracle's teacher-forced logits fed through `wrnn_nll_host`."""
    from oracle import wavernn_oracle as O
    from wavernn_amd import _lib
    from wavernn_amd.batch import score_corpus
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.score import prepare_targets
    from wavernn_amd.synthetic import random_state_dict, random_mel
    hp = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
              hop_length=128, sample_rate=16000)
    sd = random_state_dict(71, mode='MOL', **hp)
    model = WaveRNN(**hp, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    mel, steps = random_mel(72, 3), 3 * 128
    wav = short_wave(steps, 11)
    m = O.pad_tensor(mel.T[None], 2, 'both')[0].T
    mels_up, aux_up = O.upsample_network(sd, m, hp['upsample_factors'], 2)
    x = prepare_targets(wav, 'MOL')[1]
    ref = _lib.nll_host('MOL', oracle_forced_logits(sd, mels_up[None], aux_up[None], x), x[None])[0][0]
    bound = bound_of('MOL')
    for algo, kernel in (('auto', 'wrnn_generic_kernel'), ('tile', 'wrnn_tile_kernel')):
        r = score_corpus(model, [torch.from_numpy(mel).unsqueeze(0)] * 2, [wav, wav[:200]], per_step=True, algo=algo)
        assert model.last_loop_kernel == kernel, (algo, model.last_loop_kernel)
        err = max(float(np.abs(r[0]['per_step'] - ref).max()), float(np.abs(r[1]['per_step'] - ref[:200]).max()))
        print(f'{kernel}: max per-step |ours - oracle| = {err:.3e} (bound {bound:.3e})')
        assert r[0]['steps'] == steps and r[1]['steps'] == 200 and err <= bound


# ---- masks, pruning, generation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_a_short_waveform_counts_its_own_length(gpu, mode):
    """A `wav` shorter than N * hop counts len(wav) steps -- and a longer one N * hop --; the values are those of the full utterance's first steps."""
    model, bound = shipped_model(gpu, mode), bound_of(mode)
    mels, wavs = fixture_utterances()
    full = corpus_scores(gpu, mode)[0][0]['per_step']
    n = 9 * HOP - 1000
    r = model.score(mels[0], wavs[0][:n], mu_law=True, per_step=True)
    assert r['steps'] == n and r['per_step'].shape == (n,)
    assert float(np.abs(r['per_step'] - full[:n]).max()) <= bound
    assert r['nll_sum'] == pytest.approx(r['per_step'].astype(np.float64).sum(), rel=1e-12)
    r = model.score(mels[0], np.concatenate([wavs[0], wavs[0][:50]]), mu_law=True, per_step=True)
    assert r['steps'] == 9 * HOP and float(np.abs(r['per_step'] - full).max()) <= bound


def test_pruning_sweep(gpu):
    """`score_at_sparsities` at 0 and 0.95 (Linear layers too) on two 9-frame utterances: sparsity 0 is the dense score; the 0.95 entry ran on
    wrnn_sparse_kernel and agrees with the dense kernels on the same masked weights (`algo='chain'`); the caller's model is left alone."""
    from wavernn_amd.batch import score_corpus
    from wavernn_amd.prune import block_prune_state_dict, score_at_sparsities
    from wavernn_amd.synthetic import random_state_dict, random_mel
    model, bound = shipped_model(gpu, 'MOL'), bound_of('MOL')
    mels = [torch.from_numpy(random_mel(150 + u, 9)).unsqueeze(0) for u in range(2)]
    wavs = [short_wave(9 * HOP, 20 + u) for u in range(2)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    dense = score_corpus(model, mels, wavs)
    dense_mean = sum(r['nll_sum'] for r in dense) / sum(r['steps'] for r in dense)
    sweep = score_at_sparsities(model, mels, wavs, (0.0, 0.95), linear=True)
    assert [z for z, _, _ in sweep] == [0.0, 0.95]
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert abs(sweep[0][1] - dense_mean) <= bound and sweep[0][2] == model.last_loop_kernel
    assert sweep[1][2] == 'wrnn_sparse_kernel', sweep[1]
    pruned, _ = block_prune_state_dict(random_state_dict(12, mode='MOL'), 0.95, (16, 1), linear=True)
    masked = shipped_model(gpu, 'MOL', sd=pruned, key='pruned')
    on_dense = score_corpus(masked, mels, wavs, algo='chain')
    assert masked.last_loop_kernel == 'wrnn_chain_kernel'
    masked_mean = sum(r['nll_sum'] for r in on_dense) / sum(r['steps'] for r in on_dense)
    print(f'dense {dense_mean:.6f}; 95 % sparse: wrnn_sparse_kernel {sweep[1][1]:.6f}, wrnn_chain_kernel {masked_mean:.6f}')
    assert abs(sweep[1][1] - masked_mean) <= bound


def test_generation_is_untouched_by_scoring(gpu, tmp_path):
    """`generate()` on mol_unbatched_24f before and after a `score()` on the same model object: both return the fixture's waveform -- scoring leaves
    nothing behind in the engine or its workspace."""
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED
    cfg, g = load_case('mol_unbatched_24f')
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(cfg['wseed'], mode='MOL').items()}, strict=True)
    model = model.to(gpu)
    mel = torch.tensor(random_mel(cfg['mseed'], cfg['frames'])).unsqueeze(0)

    def gen():
        torch.manual_seed(cfg['seed'])
        return model.generate(mel, tmp_path / 'o.wav', cfg['batched'], cfg['target'], cfg['overlap'], cfg['mu_law'])
    first = gen()
    assert np.abs(first - g['out']).max() <= MOL_TOL
    r = model.score(fixture_utterances()[0][2], fixture()['wav2'])          # (the fixture's 24-frame utterance: its own mel, the same weights)
    assert r['steps'] == 24 * HOP and model.training
    assert abs(r['nll_mean'] - float(fixture()['mol_nll_mean'][2])) <= bound_of('MOL')
    second = gen()
    assert second.shape == first.shape and np.abs(second - g['out']).max() <= MOL_TOL
