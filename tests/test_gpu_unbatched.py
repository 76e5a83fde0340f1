"""Unbatched generation of a list of utterances on the GPU (-m gpu): `wrnn_post_chunk` against its host form, `batch.generate_unbatched` against
`WaveRNN.generate(batched=False)` of every utterance alone -- whole, and streamed in step slices --, `WaveRNN.generate_stream`, the reference's own
unbatched waveforms (tests/golden/*_unbatched_24f.npz), the block-sparse kernel and a kernel that does not continue a call.  Mels of 21-29 frames:
T <= 7975 steps, some 70 ms per loop call."""
import warnings

import numpy as np
import pytest
import torch

import unbatched_cases as U
from helpers import MOL_TOL, case_mel, load_case

pytestmark = pytest.mark.gpu

HOP = 275
FRAMES17 = [21 + (5 * k) % 9 for k in range(17)]        # 21 .. 29, ragged, 17 of them: one more than a 16-segment group
SEEDS17 = [4100 + 7 * k for k in range(17)]


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()          # fails loudly if the HIP extension is missing
    return torch.device('cuda', 0)


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', U.ROWS, ids=['row-null', 'row-permuted'])
@pytest.mark.parametrize('kind', ['mol', 'raw_lut', 'raw'])
def test_device_form_equals_host_form_bit_for_bit(gpu, kind, row):
    """`wrnn_post_chunk` == `wrnn_post_chunk_host` on the inputs of tests/test_post_chunk_host.py, for both outputs, over every hard range."""
    from wavernn_amd import _lib
    from wavernn_amd.post import chunk_host_tables, chunk_on_device
    seg, mu_law = U.segments(kind)
    tail, lut = chunk_host_tables(U.HOP, U.C, mu_law)
    d_seg, d_wl = torch.from_numpy(seg).to(gpu), torch.from_numpy(U.WAVE_LEN).to(gpu)
    d_row = None if row is None else torch.from_numpy(row).to(gpu)
    for name in sorted(U.RANGES):
        for t0, t1 in U.RANGES[name]:
            w = t1 - t0
            h64, h32 = _lib.post_chunk_host(seg, U.WAVE_LEN, t0, t1, tail, lut, row=row, want32=True)
            o64 = torch.full((3 * w + 5,), 7.0, dtype=torch.float64, device=gpu)        # (5 spare elements: nothing is written past n * (t1 - t0))
            o32 = torch.full((3 * w + 5,), 7.0, dtype=torch.float32, device=gpu)
            chunk_on_device(d_seg, d_wl, t0, t1, U.HOP, U.C, mu_law, out64=o64, out32=o32, row=d_row, min_wave_len=int(U.WAVE_LEN.min()))
            g64, g32 = o64.cpu().numpy(), o32.cpu().numpy()
            assert np.array_equal(g64[:3 * w].reshape(3, w), h64), (name, t0, t1)
            assert np.array_equal(g32[:3 * w].reshape(3, w), h32), (name, t0, t1)
            assert (g64[3 * w:] == 7.0).all() and (g32[3 * w:] == 7.0).all()
            only32 = torch.full((3 * w,), 7.0, dtype=torch.float32, device=gpu)            # one output alone
            chunk_on_device(d_seg, d_wl, t0, t1, U.HOP, U.C, mu_law, out32=only32, row=d_row)
            assert np.array_equal(only32.cpu().numpy().reshape(3, w), h32)
    with pytest.raises(ValueError, match='operands could not be broadcast'):             # the reference's ValueError, raised by the wrapper
        chunk_on_device(d_seg, d_wl, 0, 8, U.HOP, U.C, mu_law, out64=o64, min_wave_len=U.TAIL_LEN - 1)
    with pytest.raises(_lib.WrnnError, match='bad step range'):
        chunk_on_device(d_seg, d_wl, 8, 8, U.HOP, U.C, mu_law, out64=o64)


# ------------------------------------------------------------------------------------------------------------------------------
_MODELS, _ALONE = {}, {}


def _model(gpu, mode, wseed=61, prune=0.0):
    key = (mode, wseed, prune)
    if key not in _MODELS:
        from wavernn_amd.model import WaveRNN
        from wavernn_amd.synthetic import SHIPPED, random_state_dict
        sd = random_state_dict(wseed, mode=mode)
        if prune:
            from wavernn_amd.prune import block_prune_state_dict
            sd = block_prune_state_dict(sd, prune, (16, 1), linear=True)[0]
        model = WaveRNN(**SHIPPED, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        _MODELS[key] = model.to(gpu)
    return _MODELS[key]


def _mels(frames, base=3300):
    from wavernn_amd.synthetic import random_mel
    return [torch.from_numpy(random_mel(base + k, f)).unsqueeze(0) for k, f in enumerate(frames)]


def _alone(model, key, mels, seeds, mu_law, tmp_path):
    """`generate(batched=False)` of every utterance alone under 'library' noise with noise_seed = seeds[u] -- once per key, never modified"""
    if key not in _ALONE:
        outs, kernels = [], set()
        src, seed = model.noise_source, model.noise_seed
        try:
            model.noise_source = 'library'
            for u, m in enumerate(mels):
                model.noise_seed = seeds[u]
                y = model.generate(m, tmp_path / f'alone{u}.wav', False, 11000, 550, mu_law)
                y.setflags(write=False)
                outs.append(y)
                kernels.add(model.last_loop_kernel)
        finally:
            model.noise_source, model.noise_seed = src, seed
        _ALONE[key] = (outs, kernels)
    return _ALONE[key]


KINDS = {'mol': ('MOL', False), 'raw-mulaw': ('RAW', True), 'raw-linear': ('RAW', False)}


@pytest.mark.parametrize('n', [1, 3, 17])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_list_equals_every_utterance_alone_whole_and_streamed(gpu, kind, n, tmp_path):
    """Shipped dims, random weights, 'library' noise: every waveform of `generate_unbatched` is that of `generate(batched=False)` alone with
    noise_seed = seeds[u], on wrnn_chain_kernel on both sides; the same streamed in slices of 997 / 1651 / more than T steps, whose chunks concatenate
    to the return value."""
    from wavernn_amd.batch import generate_unbatched
    mode, mu_law = KINDS[kind]
    model = _model(gpu, mode)
    mels = _mels(FRAMES17)
    alone, kernels = _alone(model, kind, mels, SEEDS17, mu_law, tmp_path)
    assert kernels == {'wrnn_chain_kernel'}, kernels
    mels, seeds = mels[:n], SEEDS17[:n]
    wave_len = [(f - 1) * HOP for f in FRAMES17[:n]]
    for chunk_steps in (None, 997, 1651, 10 ** 6):
        calls, tm = [], {}
        outs = generate_unbatched(model, mels, mu_law, seeds, chunk_steps=chunk_steps, timings=tm,
                                  on_chunk=lambda u, start, s: calls.append((u, start, s)))
        assert model.last_loop_kernel == 'wrnn_chain_kernel', model.last_loop_kernel
        assert len(outs) == n
        for u in range(n):
            assert outs[u].dtype == np.float64 and outs[u].shape == alone[u].shape
            diff = np.flatnonzero(outs[u] != alone[u])
            print(f'{kind} n={n} chunk_steps={chunk_steps} u={u}: {diff.size} samples differ' + (f', first at {diff[0]}, max |d| {np.abs(outs[u] - alone[u]).max():.3e}' if diff.size else ''))
            assert diff.size == 0, (chunk_steps, u, diff.size)
            mine = [(start, s) for v, start, s in calls if v == u]
            assert [start for start, _ in mine] == sorted(start for start, _ in mine) and np.array_equal(np.concatenate([s for _, s in mine]), outs[u])
        T = max(FRAMES17[:n]) * HOP
        k = T if chunk_steps is None else min(chunk_steps, T)
        assert [start for _, start, _ in calls] == sorted(start for _, start, _ in calls)            # step order first
        assert len(calls) == sum(1 for t0 in range(0, T, k) for w in wave_len if t0 < w)
        assert tm['slices'] == -(-T // k) and tm['loop_ms'] > 0 and tm['first_chunk_ms'] > 0
    outs32 = generate_unbatched(model, mels, mu_law, seeds, chunk_steps=997, dtype=np.float32)
    assert all(o.dtype == np.float32 and np.array_equal(o, a.astype(np.float32)) for o, a in zip(outs32, alone))


@pytest.mark.parametrize('name', ['mol_unbatched_24f', 'raw_unbatched_24f'])
def test_reference_unbatched_waveforms_through_the_list_path(gpu, name):
    """The two unbatched fixtures -- what the reference's own `generate(batched=False)` returned after `torch.manual_seed(seed)` -- through
    `generate_unbatched(noise_source='cpu')`, between two other utterances, whole and streamed: RAW identical, MoL within MOL_TOL (the bars of
    test_generate_end_to_end)."""
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.synthetic import random_mel
    cfg, g = load_case(name)
    model = _model(gpu, cfg['mode'], wseed=cfg['wseed'])
    mels = [random_mel(701, 22), case_mel(cfg, g), random_mel(702, 21)]
    state = torch.get_rng_state()
    for chunk_steps in (None, 997):
        out = generate_unbatched(model, mels, cfg['mu_law'], [311, cfg['seed'], 312], noise_source='cpu', chunk_steps=chunk_steps)[1]
        assert out.dtype == np.float64 and out.shape == g['out'].shape
        err = np.abs(out - g['out']).max()
        print(f'{name} chunk_steps={chunk_steps}: max |out - reference| = {err:.3e}, {np.count_nonzero(out != g["out"])} samples differ')
        if cfg['mode'] == 'RAW':
            assert np.array_equal(out, g['out']), f'{np.count_nonzero(out != g["out"])} samples differ'
        else:
            assert err <= MOL_TOL, err
    assert torch.equal(state, torch.get_rng_state())                    # private generators: the global one is untouched


@pytest.mark.parametrize('noise', ['library', 'cpu'])
@pytest.mark.parametrize('kind', ['mol', 'raw-mulaw'])
def test_generate_stream_concatenates_to_generate(gpu, kind, noise, tmp_path):
    """`generate_stream`: at least 3 chunks, whose concatenation is what `generate(batched=False)` returns under the same noise source; 'cpu' leaves
    torch's global generator where `generate` leaves it."""
    mode, mu_law = KINDS[kind]
    model = _model(gpu, mode)
    mel = _mels([29], base=3400)[0]
    src, seed = model.noise_source, model.noise_seed
    try:
        model.noise_source, model.noise_seed = noise, 977
        torch.manual_seed(55)
        whole = model.generate(mel, tmp_path / 'whole.wav', False, 11000, 550, mu_law)
        after_whole = torch.get_rng_state()
        model.train()
        torch.manual_seed(55)
        chunks = list(model.generate_stream(mel, mu_law))
        assert model.training and model.last_loop_kernel == 'wrnn_chain_kernel'
        assert len(chunks) >= 3 and [len(c) for c in chunks] == [2200, 2200, 2200, 28 * HOP - 6600]
        got = np.concatenate(chunks)
        assert got.dtype == np.float64 and got.shape == whole.shape
        assert np.array_equal(got, whole), f'{np.count_nonzero(got != whole)} samples differ'
        assert torch.equal(after_whole, torch.get_rng_state())
        torch.manual_seed(55)
        odd = list(model.generate_stream(mel, mu_law, chunk_steps=1651, dtype=np.float32))
        assert np.array_equal(np.concatenate(odd), whole.astype(np.float32)) and len(odd) == 5
    finally:
        model.noise_source, model.noise_seed = src, seed


def test_block_sparse_kernel_streams_too(gpu, tmp_path):
    """A 95 % block-pruned MoL model (GRUs and Linear layers), three utterances in slices of 997 steps on wrnn_sparse_kernel: chunked == unchunked ==
    every utterance alone."""
    from wavernn_amd.batch import generate_unbatched
    model = _model(gpu, 'MOL', wseed=52, prune=0.95)
    frames, seeds = [24, 29, 21], [91, 92, 93]
    mels = _mels(frames, base=3500)
    alone, kernels = _alone(model, 'mol-pruned', mels, seeds, False, tmp_path)
    assert kernels == {'wrnn_sparse_kernel'}, kernels
    whole = generate_unbatched(model, mels, False, seeds)
    assert model.last_loop_kernel == 'wrnn_sparse_kernel'
    calls = []
    chunked = generate_unbatched(model, mels, False, seeds, chunk_steps=997, on_chunk=lambda u, start, s: calls.append((u, start)))
    assert model.last_loop_kernel == 'wrnn_sparse_kernel' and len(calls) > 3 * 5
    for u in range(3):
        assert np.array_equal(chunked[u], whole[u]), (u, np.count_nonzero(chunked[u] != whole[u]))
        assert np.array_equal(chunked[u], alone[u]), (u, np.count_nonzero(chunked[u] != alone[u]))


def test_a_kernel_that_does_not_continue_a_call_delivers_whole_utterances(gpu):
    """A 256 / 256 MoL model on `algo = 'tile'` (wrnn_tile_kernel: whole calls only) with chunk_steps=997: ONE warning, one chunk per utterance at the
    end, and the audio of the call without chunk_steps."""
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel, random_state_dict
    hp = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
              hop_length=128, sample_rate=16000)
    sd = random_state_dict(71, mode='MOL', **hp)
    model = WaveRNN(**hp, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    model.loop_algo = 'tile'
    frames, seeds = [23, 30, 21], [5, 6, 7]
    mels = [torch.tensor(random_mel(3600 + k, f, n_mels=80)).unsqueeze(0) for k, f in enumerate(frames)]
    whole = generate_unbatched(model, mels, False, seeds, max_utterances=2)
    assert model.last_loop_kernel == 'wrnn_tile_kernel', model.last_loop_kernel
    calls = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        chunked = generate_unbatched(model, mels, False, seeds, chunk_steps=997, max_utterances=2,
                                     on_chunk=lambda u, start, s: calls.append((u, start, len(s))))
    said = [w for w in caught if 'does not continue a call' in str(w.message)]
    assert len(said) == 1 and 'wrnn_tile_kernel' in str(said[0].message), [str(w.message) for w in caught]          # two groups, one warning
    assert calls == [(1, 0, 29 * 128), (0, 0, 22 * 128), (2, 0, 20 * 128)]
    for u in range(3):
        assert whole[u].shape == ((frames[u] - 1) * 128,) and np.abs(whole[u]).max() > 0.01
        assert np.array_equal(chunked[u], whole[u]), u
