"""LIVE streaming from the loop kernels that are launched once for all steps (wrnn_generic_kernel and the four tile kernels), on the GPU: a watched call
(`wrnn_generate_segments_watched`) computes the plain call's bits and every progress value it publishes is true -- what a copy launched after the look
reads of out[:, :m] is final --, and `generate_unbatched(live=True)` / `generate_stream(live=True)` deliver the chunks of the sliced path while the
kernel runs.  Model: rnn = fc = 256, hop 128 (tests/test_gpu_unbatched.py's tile test); mels of 21-30 frames, T <= 3,712: a few tenths of a second of loop."""
import time
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOP = 128
HP = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
          hop_length=HOP, sample_rate=16000)
_MODELS, _COND = {}, {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _model(gpu, kind):
    """kind: 'mol' | 'raw' (9 bits) | 'pruned' (MoL, 95 % of the 16x1 blocks of the GRU and Linear matrices pruned) -- built once"""
    if kind not in _MODELS:
        from wavernn_amd.model import WaveRNN
        from wavernn_amd.synthetic import random_state_dict
        mode = 'RAW' if kind == 'raw' else 'MOL'
        sd = random_state_dict(71, mode=mode, **HP)
        if kind == 'pruned':
            from wavernn_amd.prune import block_prune_state_dict
            sd = block_prune_state_dict(sd, 0.95, (16, 1), linear=True)[0]
        model = WaveRNN(**HP, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        _MODELS[kind] = model.to(gpu).eval()
    return _MODELS[kind]


def _mels(frames, base=3700):
    from wavernn_amd.synthetic import random_mel
    return [torch.tensor(random_mel(base + k, f, n_mels=80)).unsqueeze(0) for k, f in enumerate(frames)]


def _conditioning(gpu, kind, frames):
    """(mels_up, aux, seg_pos, seg_lim, T) of the utterances as one unfolded segment each -- once per (model, frames), never modified"""
    key = (kind, tuple(frames))
    if key not in _COND:
        from wavernn_amd.batch import _unbatched_plan
        model = _model(gpu, kind)
        with torch.no_grad():
            ups, auxs = zip(*[model.conditioning(m.to(gpu))[:2] for m in _mels(frames)])
        plan = _unbatched_plan(frames, HOP)
        _COND[key] = (torch.cat(ups).contiguous(), torch.cat(auxs).contiguous(), plan.seg_pos, plan.seg_lim, plan.T)
    return _COND[key]


FRAMES3 = [30, 23, 27]
FRAMES17 = [30, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 21, 24, 27, 30, 22, 26]
#: (algo, clusters, model, frames, kernel)
WATCHED = {
    'generic-auto': ('auto', 0, 'mol', FRAMES3, 'wrnn_generic_kernel'),
    'tile': ('tile', 0, 'mol', FRAMES3, 'wrnn_tile_kernel'),
    'tile-width4': ('tile', 4, 'mol', FRAMES3, 'wrnn_tile_wide_kernel'),
    'tile_bf16': ('tile_bf16', 0, 'mol', FRAMES3, 'wrnn_tile_bf16_kernel'),
    'tile_sparse-pruned': ('tile_sparse', 0, 'pruned', FRAMES3, 'wrnn_tile_sparse_kernel'),
    'tile-17-segments': ('tile', 0, 'mol', FRAMES17, 'wrnn_tile_kernel'),
    'tile-raw9': ('tile', 0, 'raw', FRAMES3, 'wrnn_tile_kernel'),
}
EVERY = 16


@pytest.mark.parametrize('case', sorted(WATCHED))
def test_watched_call_same_bits_and_visible_when_promised(gpu, case):
    algo, clusters, kind, frames, kernel = WATCHED[case]
    model = _model(gpu, kind)
    eng = model._loop_engine()
    mels_up, aux, seg_pos, seg_lim, T = _conditioning(gpu, kind, frames)
    n = len(frames)
    ids = np.arange(900, 900 + n, dtype=np.uint64)
    kw = dict(algo=algo, clusters=clusters, noise_seed=77, noise_seg_id=ids)
    plain = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, **kw)
    assert eng.last_loop_kernel() == kernel
    plain = plain.cpu().numpy()

    n_words = eng.watch_words(n, T, algo=algo, clusters=clusters)
    assert n_words == (n if kernel == 'wrnn_generic_kernel' else (n + 15) // 16)
    main, side = torch.cuda.current_stream(gpu), torch.cuda.Stream(gpu, priority=-1)      # (a hardware queue the main stream's kernel is never in)
    words = torch.zeros(n_words, dtype=torch.int32, device=gpu)
    out = torch.full((n, T), float('nan'), dtype=torch.float32, device=gpu)
    words_pin = torch.zeros(n_words, dtype=torch.int32, pin_memory=True)
    snap_pin = torch.empty(n * T, dtype=torch.float32, pin_memory=True)
    zeroed, done = torch.cuda.Event(), torch.cuda.Event()
    zeroed.record(main)
    side.wait_event(zeroed)
    eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, check=False, out=out, watch=(words, EVERY), **kw)
    done.record(main)

    seen, snaps = [], []
    while True:
        last = done.query()                             # (asked BEFORE the look: the look after the end must read T)
        with torch.cuda.stream(side):
            words_pin.copy_(words, non_blocking=True)
        side.synchronize()
        m = int(words_pin.min())
        seen.append(m)
        if m > 0 and (not snaps or snaps[-1][0] != m):
            with torch.cuda.stream(side):               # launched after the look: what the words promise
                snap_pin[:n * m].view(n, m).copy_(out[:, :m], non_blocking=True)
            side.synchronize()
            snaps.append((m, snap_pin[:n * m].view(n, m).clone()))
        if last:
            break
        time.sleep(0.001)
    eng.status()
    assert eng.last_loop_kernel() == kernel
    loop_ms = eng.last_loop_ms()
    final = out.cpu().numpy()
    print(f'{case}: {kernel} n={n} T={T} loop {loop_ms:.1f} ms = {loop_ms * 1e3 / T:.1f} us/step, {len(seen)} looks, {len(snaps)} snapshots, '
          f'first m > 0: {next((m for m in seen if m), None)}')
    # (c) the plain call's bits
    assert np.array_equal(final, plain), f'{np.count_nonzero(final != plain)} samples differ from the plain call'
    # (a) the observed values
    assert seen == sorted(seen), seen
    assert all(m % EVERY == 0 or m == T for m in seen), [m for m in seen if m % EVERY and m != T]
    assert seen[-1] == T, seen[-5:]
    # (b) every snapshot is final
    for m, snap in snaps:
        got = snap.numpy()
        assert np.array_equal(got, final[:, :m]), f'word = {m}: {np.count_nonzero(got != final[:, :m])} of the promised samples were not final'
    # (d) it arrived while the kernel ran
    assert any(0 < m < T for m in seen), f'publication arrived only at the end: {len(seen)} looks over {loop_ms:.1f} ms saw {sorted(set(seen))}'


def test_a_watched_call_is_refused_where_it_cannot_run(gpu):
    from wavernn_amd import _lib
    model = _model(gpu, 'mol')
    eng = model._loop_engine()
    mels_up, aux, seg_pos, seg_lim, T = _conditioning(gpu, 'mol', FRAMES3)
    words = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(_lib.WrnnError, match='progress_words = 1'):
        eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, watch=(words, 16))          # wrnn_generic_kernel: three words
    with pytest.raises(_lib.WrnnError, match='progress_every = 0'):
        eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, algo='tile', watch=(words, 0))


LIVE_LIST = {'tile': ('mol', 0, False), 'tile-width4': ('mol', 4, False), 'tile-raw9-mulaw': ('raw', 0, True)}


@pytest.mark.parametrize('case', sorted(LIVE_LIST))
def test_list_live(gpu, case):
    from wavernn_amd.batch import generate_unbatched
    kind, width, mu_law = LIVE_LIST[case]
    model = _model(gpu, kind)
    model.loop_algo, model.tile_width = 'tile', width
    kernel = 'wrnn_tile_wide_kernel' if width else 'wrnn_tile_kernel'
    try:
        frames, seeds = [23, 30, 21], [5, 6, 7]
        mels = _mels(frames, base=3600)
        whole = generate_unbatched(model, mels, mu_law, seeds, max_utterances=2)
        assert model.last_loop_kernel == kernel
        calls, tm = [], {}
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            live = generate_unbatched(model, mels, mu_law, seeds, chunk_steps=997, max_utterances=2, live=True, timings=tm,
                                      on_chunk=lambda u, start, s: calls.append((u, start, len(s))))
        assert not [str(w.message) for w in caught if 'does not continue a call' in str(w.message)]
        assert model.last_loop_kernel == kernel
        print(f'{case}: first chunk after {tm["first_chunk_ms"]:.1f} ms, loop {tm["loop_ms"]:.1f} ms, {tm["slices"]} slices')
        for u, f in enumerate(frames):
            wl = (f - 1) * HOP
            mine = [(s, ln) for v, s, ln in calls if v == u]
            assert [s for s, _ in mine] == list(range(0, wl, 997)) and len(mine) >= 3, mine
            assert sum(ln for _, ln in mine) == wl
            assert live[u].shape == (wl,) and np.abs(live[u]).max() > 0.01
            assert np.array_equal(live[u], whole[u]), (u, np.count_nonzero(live[u] != whole[u]))
        # within a slice the group's order: group one = utterances 1, 0 (longest first), then group two = utterance 2
        assert [u for u, s, _ in calls if s == 0] == [1, 0, 2]
        assert tm['slices'] == -(-29 * HOP // 997) + -(-20 * HOP // 997)
    finally:
        model.loop_algo, model.tile_width = 'auto', 0


def test_one_utterance_live(gpu, tmp_path):
    model = _model(gpu, 'mol')
    model.loop_algo = 'tile'
    src, seed = model.noise_source, model.noise_seed
    try:
        model.noise_source, model.noise_seed = 'library', 977
        mel = _mels([29], base=3400)[0]
        whole = model.generate(mel, tmp_path / 'whole.wav', False, 11000, 550, False)
        chunks = list(model.generate_stream(mel, False, chunk_steps=1651, live=True))
        assert model.last_loop_kernel == 'wrnn_tile_kernel'
        assert [len(c) for c in chunks] == [1651, 1651, 28 * HOP - 2 * 1651]
        assert np.array_equal(np.concatenate(chunks), whole)
    finally:
        model.noise_source, model.noise_seed, model.loop_algo = src, seed, 'auto'


def test_live_on_a_kernel_that_continues_a_call_is_the_sliced_path(gpu):
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import SHIPPED, random_mel, random_state_dict
    sd = random_state_dict(61, mode='MOL')
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    mels, seeds = [torch.from_numpy(random_mel(3300 + k, f)).unsqueeze(0) for k, f in enumerate([24, 29, 21])], [91, 92, 93]
    runs = {}
    for live in (False, True):
        calls = []
        outs = generate_unbatched(model, mels, False, seeds, chunk_steps=997, live=live, on_chunk=lambda u, start, s: calls.append((u, start, s)))
        assert model.last_loop_kernel == 'wrnn_chain_kernel'
        runs[live] = (outs, calls)
    (a, ca), (b, cb) = runs[False], runs[True]
    assert len(ca) > 3 * 5 and [(u, s) for u, s, _ in ca] == [(u, s) for u, s, _ in cb]
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(ca, cb))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_consumer_that_stops_looking(gpu, tmp_path):
    """The generator is closed after its first chunk: the kernel goes on to its end on its own (it waits for nobody), and the device serves the next
    call as usual."""
    model = _model(gpu, 'mol')
    model.loop_algo = 'tile'
    src, seed = model.noise_source, model.noise_seed
    try:
        model.noise_source, model.noise_seed = 'library', 978
        mel = _mels([30], base=3450)[0]
        usual = model.generate(mel, tmp_path / 'a.wav', False, 11000, 550, False)
        gen = model.generate_stream(mel, False, chunk_steps=500, live=True)
        first = next(gen)
        gen.close()
        assert np.array_equal(first, usual[:500])
        again = model.generate(mel, tmp_path / 'b.wav', False, 11000, 550, False)
        assert model.last_loop_kernel == 'wrnn_tile_kernel'
        assert np.array_equal(again, usual)
        torch.cuda.synchronize()
    finally:
        model.noise_source, model.noise_seed, model.loop_algo = src, seed, 'auto'
