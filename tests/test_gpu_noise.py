"""The library's own sampling noise on the device (wrnn_options.noise_lib; csrc/wrnn_noise.hip, csrc/wrnn_philox.h): the fill kernel against the host
form, and every loop kernel drawing its noise itself against the same call fed the tensor `wrnn_noise_fill` writes -- bit for bit: the loop kernels
are the same, only where their noise comes from differs.

Shapes: 19 segments (two groups of <= 16, the second ragged), shipped dims and hop, 40 steps in slabs of 16 -- three slabs, the last one short, so that the
per-slab fill and `noise_t0` are exercised at two slab boundaries; 300 segments on wrnn_chain_kernel are two rounds that share one slab of noise.  The
values themselves are pinned on the CPU (tests/test_noise_host.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, SLAB, STRIDE, HOP = 19, 40, 16, 8, 275
SEED = 0x5EED0123456789AB
RTOL = 1e-6              # RAW: two logf implementations, each good to an ulp or so (6e-8), of the same float32 argument
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _ids(n):
    """n distinct 64-bit stream ids with both halves in use, in no particular order"""
    return (np.arange(n, dtype=np.uint64)[::-1] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF0000000000)


def _engine(gpu, kind):
    """LoopEngine per weight set ('MOL', 'RAW': dense shipped dims; 'MOL-pruned': GRU matrices and Linear layers 95 % block-pruned)"""
    if kind not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        from wavernn_amd.synthetic import random_state_dict
        mode = kind.split('-')[0]
        sd = random_state_dict(61, mode=mode)
        if kind.endswith('pruned'):
            from wavernn_amd.prune import block_prune_state_dict
            sd = block_prune_state_dict(sd, 0.95, (16, 1), linear=True)[0]
        _MEMO[kind] = LoopEngine(sd, mode, device=gpu)
    return _MEMO[kind]


def _cond(gpu, n, feat=80, aux=128, hop=HOP):
    key = ('cond', n, feat, aux, hop)
    if key not in _MEMO:
        rs = np.random.RandomState(4)
        L = (n * STRIDE + T + hop - 1) // hop * hop
        _MEMO[key] = (torch.from_numpy(rs.uniform(0, 1, (L, feat)).astype(np.float32)).to(gpu),
                      torch.from_numpy(rs.uniform(-1, 1, (L // hop, aux)).astype(np.float32)).to(gpu))
    return _MEMO[key]


def _both(eng, gpu, n, ids, cond=None, hop=HOP, **kw):
    """(samples with the library drawing the noise, samples of the same call fed wrnn_noise_fill's tensor, run info of the former)"""
    from wavernn_amd.rng import library_noise
    mels_up, aux = cond or _cond(gpu, n)
    noise = library_noise(eng.mode, n, 0, T, eng.n_classes, gpu, SEED, ids)
    explicit = eng.run(mels_up, aux, n, T, STRIDE, noise, hop, **kw).cpu().numpy()
    info_explicit = eng.last_run_info()
    lib = eng.run(mels_up, aux, n, T, STRIDE, None, hop, noise_seed=SEED, noise_seg_id=ids, **kw).cpu().numpy()
    info = eng.last_run_info()
    assert info == info_explicit, (info, info_explicit)
    assert np.isfinite(lib).all() and len(np.unique(lib)) > T
    return lib, explicit, info


def _same(lib, explicit):
    bad = np.argwhere(lib != explicit)
    assert bad.size == 0, f'{len(bad)} of {lib.size} samples differ from the explicit-tensor run, first at (segment, step) = {tuple(bad[0])}'


@pytest.mark.parametrize('ids', ['default-ids', 'ids'])
def test_device_fill_is_the_host_fill(gpu, ids):
    from wavernn_amd import _lib
    from wavernn_amd.rng import library_noise
    # 300 segments: with ids, two launches of <= 256 ids each
    for n in (N, 300):
        sid = _ids(n) if ids == 'ids' else None
        dev = library_noise('MOL', n, 3, T, 30, gpu, SEED, sid).cpu().numpy()
        host = _lib.noise_fill_host('MOL', n, 30, 3, T, SEED, sid)
        assert dev.shape == host.shape == (T - 3, 11 * n) and np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    for C in (512, 7):
        sid = _ids(N) if ids == 'ids' else None
        dev = library_noise('RAW', N, 3, T, C, gpu, SEED, sid).cpu().numpy()
        host = _lib.noise_fill_host('RAW', N, C, 3, T, SEED, sid)
        assert dev.shape == host.shape == (T - 3, N, C) and np.all(np.isfinite(dev)) and np.all(dev > 0)
        np.testing.assert_allclose(dev, host, rtol=RTOL, atol=0)


@pytest.mark.parametrize('algo', ['auto', 'duo', 'loop', 'stream'])
@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_library_noise_is_the_explicit_tensor(gpu, mode, algo):
    lib, explicit, info = _both(_engine(gpu, mode), gpu, N, _ids(N), algo=algo, slab_steps=SLAB)
    want = dict(auto='wrnn_chain_kernel', duo='wrnn_duo_kernel', loop='wrnn_loop_kernel', stream='wrnn_stream_kernel')[algo]
    assert info['kernel'] == want and info['launches'] == (1 if algo == 'stream' else 3) and (algo == 'stream' or info['slab_steps'] == SLAB), info
    _same(lib, explicit)


def test_library_noise_on_the_block_sparse_kernel(gpu):
    eng = _engine(gpu, 'MOL-pruned')
    for algo in ('auto', 'sparse'):
        lib, explicit, info = _both(eng, gpu, N, _ids(N), algo=algo, slab_steps=SLAB)
        assert info['kernel'] == 'wrnn_sparse_kernel' and info['launches'] == 3, info
        _same(lib, explicit)


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_two_rounds_share_a_slab_of_noise(gpu, mode):
    """300 segments on wrnn_chain_kernel (256 a round): two rounds per slab read their rows of ONE fill; with ids, the fill is two launches."""
    n = 300
    lib, explicit, info = _both(_engine(gpu, mode), gpu, n, _ids(n), algo='chain', slab_steps=SLAB)
    assert (info['kernel'], info['rounds'], info['launches']) == ('wrnn_chain_kernel', 2, 6), info
    _same(lib, explicit)
    # ... and without ids segment b has id b
    lib2, explicit2, _ = _both(_engine(gpu, mode), gpu, n, None, algo='chain', slab_steps=SLAB)
    _same(lib2, explicit2)
    _same(lib2, _both(_engine(gpu, mode), gpu, n, np.arange(n, dtype=np.uint64), algo='chain', slab_steps=SLAB)[0])
    assert not np.array_equal(lib, lib2)


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_a_continued_call_needs_only_seed_and_ids(gpu, mode):
    """[0, T) in one call == [0, 21) and [21, T): 21 is no slab boundary (slabs of 16), so the second call's first slab starts inside a slab of the first."""
    eng, ids = _engine(gpu, mode), _ids(N)
    mels_up, aux = _cond(gpu, N)
    kw = dict(slab_steps=SLAB, noise_seed=SEED, noise_seg_id=ids)
    whole = eng.run(mels_up, aux, N, T, STRIDE, None, HOP, **kw).cpu().numpy()
    out = None
    for t0, t1 in ((0, 21), (21, T)):
        out = eng.run(mels_up, aux, N, T, STRIDE, None, HOP, t_range=(t0, t1), out=out, **kw)
    assert eng.last_run_info()['launches'] == 2 + 2
    _same(out.cpu().numpy(), whole)


def test_generic_dims_draw_their_noise_too(gpu):
    """rnn 256, fc 384, 8 bits, 40 mel bins, aux 16, hop 128: wrnn_generic_kernel takes all T steps of noise from the workspace."""
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.synthetic import random_state_dict
    hp = dict(rnn_dims=256, fc_dims=384, bits=8, feat_dims=40, compute_dims=64, res_out_dims=64, res_blocks=3, upsample_factors=(4, 4, 8))
    for mode in ('RAW', 'MOL'):
        eng = LoopEngine(random_state_dict(71, mode=mode, **hp), mode, device=gpu)
        lib, explicit, info = _both(eng, gpu, 5, _ids(5), cond=_cond(gpu, 5, 40, 64, 128), hop=128)
        assert info['kernel'] == 'wrnn_generic_kernel' and info['launches'] == 1, info
        _same(lib, explicit)


def test_the_engine_refuses_a_tensor_beside_the_option(gpu):
    import ctypes
    from wavernn_amd import _lib
    eng = _engine(gpu, 'MOL')
    mels_up, aux = _cond(gpu, N)
    with pytest.raises(ValueError):
        eng.run(mels_up, aux, N, T, STRIDE, None, HOP, noise_seed=SEED, noise_seg_id=_ids(N + 1))
    o, noise = _lib.Options(noise_lib=1), torch.zeros(T, 11 * N, device=gpu)
    pos, lim = np.arange(N, dtype=np.int32) * STRIDE, np.full(N, mels_up.shape[0], np.int32)
    ws = torch.empty(eng.workspace_bytes(N, T, aux.shape[0], noise_lib=True), dtype=torch.uint8, device=gpu)
    out = torch.empty(N, T, device=gpu)
    rc = eng.lib.wrnn_generate_segments(eng._pack, N, T, pos.ctypes.data, lim.ctypes.data, mels_up.shape[0], HOP, aux.shape[0], mels_up.data_ptr(),
                                        aux.data_ptr(), noise.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), ctypes.byref(o), None)
    assert rc == _lib.ERR_ARG and b'`noise` must be NULL' in eng.lib.wrnn_last_error()


# ---- through the model: one utterance sounds the same alone and in any batch -----------------------------------------------------------------
def _model(gpu, mode):
    if ('model', mode) not in _MEMO:
        from wavernn_amd.model import WaveRNN
        from wavernn_amd.synthetic import random_state_dict, SHIPPED
        model = WaveRNN(**SHIPPED, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(61, mode=mode).items()}, strict=True)
        _MEMO[('model', mode)] = model.to(gpu)
    return _MEMO[('model', mode)]


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_an_utterance_is_the_same_alone_and_in_any_batch(gpu, mode, tmp_path):
    from wavernn_amd.batch import generate_corpus
    from wavernn_amd.fold import fold_geometry
    from wavernn_amd.synthetic import random_mel
    model = _model(gpu, mode)
    frames, seeds = (24, 22, 21), [71, 2 ** 32 + 5, 9]
    mels = [torch.from_numpy(random_mel(1700 + k, f)).unsqueeze(0) for k, f in enumerate(frames)]
    folds = [fold_geometry(f * HOP, 550, 55)[0] for f in frames]
    together = generate_corpus(model, mels, 550, 55, True, seeds, noise_source='library')
    assert model._loop_engine().last_run_info()['launches'] == model._loop_engine().last_run_info()['rounds'] * -(-660 // model._loop_engine().last_run_info()['slab_steps'])
    # chunks of whole utterances of at most max(folds) segments: every utterance a launch of its own
    split = generate_corpus(model, mels, 550, 55, True, seeds, noise_source='library', max_segments_per_launch=max(folds))
    model.noise_source = 'library'
    try:
        for u, mel in enumerate(mels):
            model.noise_seed = seeds[u]
            alone = model.generate(mel, tmp_path / f'{u}.wav', True, 550, 55, True)
            assert alone.shape == together[u].shape == split[u].shape and alone.size == (frames[u] - 1) * HOP
            assert np.array_equal(alone, together[u]) and np.array_equal(alone, split[u]), u
        assert not np.array_equal(together[0][:5000], together[1][:5000])
        # seeds count by their low 32 bits only; another seed is another utterance
        model.noise_seed = seeds[1] & 0xFFFFFFFF
        assert np.array_equal(model.generate(mels[1], tmp_path / 'low.wav', True, 550, 55, True), together[1])
        model.noise_seed = seeds[1] + 1
        assert not np.array_equal(model.generate(mels[1], tmp_path / 'other.wav', True, 550, 55, True), together[1])
    finally:
        model.noise_source, model.noise_seed = 'cpu', 0


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_generate_draws_nothing_from_torch(gpu, mode, tmp_path):
    """noise_source='library': one engine call for all T steps however small `noise_chunk_bytes` is, and torch's generators where they were."""
    from wavernn_amd.synthetic import random_mel
    model = _model(gpu, mode)
    mel = torch.from_numpy(random_mel(1800, 24)).unsqueeze(0)
    calls = []
    eng = model._loop_engine()
    run = eng.run_segments
    eng.run_segments = lambda *a, **k: (calls.append((a[5], k.get('t_range'))), run(*a, **k))[1]
    torch.manual_seed(5)
    torch.cuda.manual_seed(6)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(gpu)
    model.noise_source, model.noise_seed, chunk = 'library', 3, model.noise_chunk_bytes
    model.noise_chunk_bytes = 1 << 16
    try:
        model.generate(mel, tmp_path / 'a.wav', True, 550, 55, True)
    finally:
        model.noise_source, model.noise_seed, model.noise_chunk_bytes = 'cpu', 0, chunk
        del eng.run_segments
    assert calls == [(None, None)], calls
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(gpu), dev_state)
