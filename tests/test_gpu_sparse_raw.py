"""The 9-bit RAW mode of wrnn_sparse_kernel (`algo = 'sparse'` on a block-pruned RAW pack): fc3 as every workgroup's dense 32-row stage, the
logits as layer 16, four sampling workgroups per cluster (csrc/wrnn_sparse.hip).  Checked against the C oracle running the same pruned
weights as masked dense matrices, class index by class index.  The kernel sums the surviving columns in another order than the oracle, so
a class can differ where two classes are tied to within float32 rounding; where a test allows that, it certifies the tie from the
oracle's own logits instead of skipping it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_MEMO = {}
TIE_REL = 1e-6


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _raw_case(frames, target, overlap, linear, wseed=36, mseed=136, seed=96):
    """Inputs + the C oracle's free run and logits on 95 %-block-pruned RAW weights (memoised); `linear`: fc1 / fc2 pruned too."""
    from oracle import c_oracle as C, wavernn_oracle as O
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict, random_mel
    key = (frames, target, overlap, linear, wseed, mseed, seed)
    if key not in _MEMO:
        sd0 = random_state_dict(wseed, mode='RAW')
        sd, _ = block_prune_state_dict(sd0, 0.95, (16, 1), linear=linear)
        mel = random_mel(mseed, frames)
        m = O.pad_tensor(mel.T[None], 2, 'both')[0].T
        mels_up, aux_up = O.upsample_network(sd, m)
        aux = np.ascontiguousarray(aux_up[::275])
        B = O.num_folds(mels_up.shape[0], target, overlap)
        T, stride = target + 2 * overlap, target + overlap
        noise = np.ascontiguousarray(O.draw_noise(seed, 'RAW', B, T), np.float32)
        mels_f, aux_f, _ = O.conditioning(sd, mel, True, target, overlap)
        ref, ref_logits = C.loop(sd, 'RAW', mels_f, aux_f, noise, want_logits=True)
        _MEMO[key] = (sd, mels_up, aux, (B, T, stride), noise, ref, ref_logits)
    return _MEMO[key]


def _tie(logits, q):
    """fatchord_version.py:231-237 in float64 on one segment-step: True when the two largest p / q are within a relative TIE_REL."""
    lg = np.asarray(logits, np.float64)
    p = np.exp(lg - lg.max())
    p /= p.sum()
    r = np.sort(p / np.asarray(q, np.float64))
    return (r[-1] - r[-2]) <= TIE_REL * r[-1]


def _engine(sd, gpu):
    from wavernn_amd.engine import LoopEngine
    with pytest.warns(UserWarning, match='pruned GRU matrices'):
        return LoopEngine(sd, 'RAW', device=gpu)


def test_planner_raw_sparse(gpu):
    """A 95 %-pruned 9-bit RAW pack plans onto wrnn_sparse_kernel on request (16 clusters, one group each, rounds beyond 256 segments);
    `auto` keeps the dense kernels; an 8-bit RAW pack is refused with a message."""
    from wavernn_amd import _lib
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict
    sd, _ = block_prune_state_dict(random_state_dict(3, mode='RAW'), 0.95, (16, 1), linear=True)
    eng = _engine(sd, gpu)
    assert 0 < eng.sparse_blocks <= 64 and 0 < eng.sparse_fc_blocks <= 64
    for n, rounds in ((12, 1), (46, 1), (256, 1), (257, 2), (942, 4)):
        pl = eng.plan(n, 12100, algo='sparse')
        assert (pl['kernel'], pl['units_per_wg'], pl['clusters'], pl['depth'], pl['rounds']) == ('wrnn_sparse_kernel', 64, 16, 1, rounds), (n, pl)
    assert eng.plan(12, 12100)['kernel'] == 'wrnn_chain_kernel' and eng.plan(128, 12100)['kernel'] == 'wrnn_chain_kernel'
    assert eng.plan(256, 12100)['kernel'] == 'wrnn_duo_kernel'
    sd8, _ = block_prune_state_dict(random_state_dict(3, mode='RAW', bits=8), 0.95, (16, 1))
    eng8 = _engine(sd8, gpu)
    assert eng8.sparse_blocks < 0
    with pytest.raises(_lib.WrnnError, match='block-sparse kernel needs MOL or RAW with 512 classes'):
        eng8.plan(12, 100, algo='sparse')


@pytest.mark.parametrize('linear', [False, True], ids=['gru', 'gru+linear'])
def test_raw_sparse_teacher_forced_logits(gpu, linear):
    """Teacher forcing (the oracle's samples fed back): every step's 512 logits within 1e-4 of the oracle's, every class equal to the oracle's
    or a certified near-tie.  46 segments = 3 groups (the last one ragged), one slab and slabs of 97 steps."""
    sd, mels_up, aux, (B, T, stride), noise, ref, ref_logits = _raw_case(100, 550, 55, linear)
    assert B == 46
    eng = _engine(sd, gpu)
    assert (eng.sparse_fc_blocks > 0) == linear
    for slab in (0, 97):
        out, logits = eng.run(torch.from_numpy(mels_up).to(gpu), torch.from_numpy(aux).to(gpu), B, T, stride, torch.from_numpy(noise).to(gpu), 275,
                              algo='sparse', force_x=torch.from_numpy(ref), want_logits=True, slab_steps=slab)
        assert eng.last_loop_kernel() == 'wrnn_sparse_kernel'
        lg = logits.cpu().numpy()
        assert lg.shape == (T, B, 512)
        err = np.abs(lg - ref_logits).max(axis=(1, 2))
        assert err.max() <= 1e-4, f'slab {slab}: first bad step {int(np.argmax(err > 1e-4))} of {T}, max {err.max():.3e}'
        out = out.cpu().numpy()
        for b, t in np.argwhere(out != ref):
            assert _tie(ref_logits[t, b], noise[t, b]), f'slab {slab}: class differs at (b, t) = ({b}, {t}) without a near-tie'


@pytest.mark.parametrize('linear', [False, True], ids=['gru', 'gru+linear'])
@pytest.mark.parametrize('frames,target,overlap,opts', [(100, 550, 55, {}), (100, 220, 22, dict(slab_steps=97)), (300, 220, 22, {}),
                                                        (300, 220, 22, dict(slab_steps=61, tuning=256)), (100, 550, 55, 'slices')])
def test_raw_sparse_matches_oracle(gpu, frames, target, overlap, opts, linear):
    """Free-running RAW on wrnn_sparse_kernel: the class indices equal the oracle's -- 46 / 114 / 341 segments (one and two rounds, ragged
    groups), conditioning slabs (state saved and restored), every layer written through (tuning bit 8), a run continued in step slices."""
    sd, mels_up, aux, (B, T, stride), noise, ref, _ = _raw_case(frames, target, overlap, linear)
    eng = _engine(sd, gpu)
    args = (torch.from_numpy(mels_up).to(gpu), torch.from_numpy(aux).to(gpu), B, T, stride)
    if opts == 'slices':
        out = None
        for t0, t1 in ((0, 200), (200, 201), (201, T)):
            out = eng.run(*args, torch.from_numpy(noise[t0:t1]).to(gpu).contiguous(), 275, algo='sparse', t_range=(t0, t1), out=out)
        out = out.cpu().numpy()
    else:
        out = eng.run(*args, torch.from_numpy(noise).to(gpu), 275, algo='sparse', **opts).cpu().numpy()
    info = eng.last_run_info()
    assert info['kernel'] == 'wrnn_sparse_kernel' and (info['units_per_wg'], info['clusters'], info['depth']) == (64, 16, 1), info
    assert info['rounds'] == -(-(-(-B // 16)) // 16)
    bad = np.argwhere(out != ref)
    assert bad.size == 0, f'{len(bad)} samples differ, first at (b, t) = {tuple(bad[0])}'


def _waveforms(model, mels, loop_algo, mel_in_loop, path):
    from wavernn_amd.batch import generate_corpus
    model.loop_algo, model.mel_in_loop = loop_algo, mel_in_loop
    torch.manual_seed(81)
    one = model.generate(mels[0], path / f'{loop_algo}.wav', True, 550, 55, True)
    kernel_one = model.last_loop_kernel
    segs, plan = generate_corpus(model, mels, 550, 55, True, [91 + u for u in range(len(mels))], return_segments=True)
    return np.asarray(one, np.float64), segs, kernel_one, model._loop_engine().last_run_info()['kernel']


@pytest.mark.parametrize('mel_in_loop', [None, True], ids=['mel-default', 'mel-in-loop'])
def test_raw_sparse_model_level(gpu, mel_in_loop, tmp_path):
    """WaveRNN(mode='RAW') on pruned weights (GRUs + Linear layers, the notebook's recipe) with `loop_algo = 'sparse'`: `generate()` (batched)
    and `generate_corpus()` give the waveforms `loop_algo = 'duo'` gives.  `mel-in-loop`: the last up-sampling stage formed inside both
    loop kernels (wrnn_options.mel_stage = 1)."""
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED
    sd, _ = block_prune_state_dict(random_state_dict(37, mode='RAW'), 0.95, (16, 1), linear=True)
    model = WaveRNN(**SHIPPED, mode='RAW')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    mels = [torch.from_numpy(random_mel(1300 + u, f)).unsqueeze(0) for u, f in enumerate((60, 41, 77))]
    with pytest.warns(UserWarning, match='pruned GRU matrices'):
        a = _waveforms(model, mels, 'sparse', mel_in_loop, tmp_path)
    b = _waveforms(model, mels, 'duo', mel_in_loop, tmp_path)
    assert a[2] == a[3] == 'wrnn_sparse_kernel' and b[2] == b[3] == 'wrnn_duo_kernel'
    assert np.array_equal(a[0], b[0]), f'generate(): {np.count_nonzero(a[0] != b[0])} samples differ'
    assert np.array_equal(a[1], b[1]), f'generate_corpus(): {np.count_nonzero(a[1] != b[1])} segment samples differ'


def test_raw_sparse_config5_full_size(gpu):
    """Config 5's shape in RAW: 16 x 641-frame utterances = 256 segments x 12,100 steps, GRUs and Linear layers 95 % block-pruned, through
    `generate_corpus` on wrnn_sparse_kernel with parity noise, against the C oracle per utterance.  Expected identical; a divergence must be
    a certified near-tie in the oracle's own logits at the first diverging step of its segment, with every sample before it identical."""
    from helpers import oracle_utterance, pruned_state_dict
    from oracle import c_oracle as C, wavernn_oracle as O
    from wavernn_amd.batch import generate_corpus
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel, SHIPPED
    sd = pruned_state_dict('RAW', 0, 0.95, True)
    model = WaveRNN(**SHIPPED, mode='RAW')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    model.loop_algo = 'sparse'
    NU = 16
    mels = [torch.from_numpy(random_mel(1234 + u, 641)).unsqueeze(0) for u in range(NU)]
    with pytest.warns(UserWarning, match='pruned GRU matrices'):
        segs, plan = generate_corpus(model, mels, 11000, 550, True, [77 + u for u in range(NU)], return_segments=True)
    eng = model._loop_engine()
    info = eng.last_run_info()
    print(f'config 5 RAW: {info} {eng.last_loop_ms():.1f} ms')
    assert plan.n_segments == 256 and plan.T == 12100
    assert info['kernel'] == 'wrnn_sparse_kernel' and (info['clusters'], info['depth'], info['rounds']) == (16, 1, 1)
    for u in range(NU):
        ref = oracle_utterance('RAW', 0, 0.95, 1234 + u, 77 + u, 641, want_cond=False, sd=sd, linear=True)['ref']
        got = segs[plan.first[u]:plan.first[u] + plan.folds[u]].astype(np.float32)
        bad = np.argwhere(got != ref)
        if bad.size == 0:
            continue
        b = int(bad[np.argmin(bad[:, 1]), 0])
        t = int(bad[bad[:, 0] == b][:, 1].min())
        print(f'utterance {u}: first divergence at segment {b}, step {t}')
        assert np.array_equal(got[:, :t], ref[:, :t])
        # the oracle's logits and noise at that step (helpers.oracle_utterance's inputs)
        cond = oracle_utterance('RAW', 0, 0.95, 1234 + u, 77 + u, 641, want_cond=True, sd=sd, linear=True)
        mels_f, aux_f, _ = O.conditioning(sd, random_mel(1234 + u, 641), True, 11000, 550)
        nz = cond['noise'][:t + 1]
        _, lg = C.loop(sd, 'RAW', mels_f[:, :t + 1], aux_f[:, :t + 1], nz, want_logits=True)
        assert _tie(lg[t, b], nz[t, b]), f'utterance {u}: segment {b} step {t} differs without a near-tie'
