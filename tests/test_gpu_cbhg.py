"""Tacotron's encoder and post-net as HIP kernels behind the C ABI (-m gpu): `wrnn_taco_encode` / `wrnn_taco_postnet`
(csrc/wrnn_cbhg.hip) against the mirror `wavernn_amd.tacotron.TacotronInference` evaluated in float64 on the CPU.

Yardstick.  e_ref (per output) is the larger of two float32 errors against that float64 result, taken at the longest length of each
set: the float32 CPU mirror's and the float32 torch-op path's on the device (what `generate(kernel=True)` runs without
`cbhg_kernel`).  A kernel output passes when its max error against float64 is <= 8 x e_ref at every length: the torch paths sum in
blocks, the kernels in another (also blocked) order -- the factor covers two valid float32 orders, not a wrong term: a wrong tap or
a zero-padded pool shows at >= 1e-3.  Every test prints the measured ratio."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
IDS_TEXT = 'Scientists at the CERN laboratory say they have discovered a new particle.'
TACO_TOL = 1e-6                         # tests/test_gpu_config3.py: the bound of these outputs on the torch-op path
MARGIN = 8.0
ENC_N = (1, 2, 15, 16, 17, 33, 100)     # one position, shorter than the widest conv, both sides of a 16-position tile, several tiles
POST_N = (1, 17, 200)
VARIANTS = ('plain', 'negative_bank', 'random_bnorm', 'rich')


@functools.lru_cache(maxsize=None)
def _state_dict(variant='plain'):
    """`random_tacotron_state_dict(3, shapes)` as tests/test_gpu_config3.py::_tts builds it.  'negative_bank': every
    conv1d_bank.*.bnorm.bias = -0.5, so that bank values in front of the max-pool are negative (with the plain dict none is, and a
    zero-padded pool would pass unseen).  'random_bnorm' (beyond the issue's cases): random batch-norm weight / bias / running
    statistics everywhere -- the plain dict's norms are identities, which a wrong scale / shift fold would survive.  'rich':
    `helpers.rich_tacotron_state_dict(5, shapes)` instead, the weights of tests/golden/tacotron_mirror.npz -- every bias vector (pre-net,
    highways, both directions' b_ih and b_hh of the GRUs) random in +-0.1 as well as the batch norms; in the other three every bias is zero,
    and a bias placed at a wrong offset of the device blob or added outside r * (W_hn h + b_hn) would pass."""
    from helpers import rich_tacotron_state_dict
    from wavernn_amd.synthetic import random_tacotron_state_dict
    shapes = json.load(open(os.path.join(HERE, 'golden', 'tacotron_shapes.json')))
    if variant == 'rich':
        return rich_tacotron_state_dict(5, shapes)
    sd = random_tacotron_state_dict(3, shapes)
    g = torch.Generator().manual_seed(11)
    for k in sd:
        if variant == 'negative_bank' and 'conv1d_bank' in k and k.endswith('bnorm.bias'):
            sd[k] = torch.full_like(sd[k], -0.5)
        if variant == 'random_bnorm' and 'bnorm' in k and sd[k].is_floating_point():
            r = torch.rand(sd[k].shape, generator=g)
            sd[k] = 0.5 + r if k.endswith(('running_var', 'weight')) else 0.4 * r - 0.2
    return sd


def _tts(dev, variant='plain', double=False, **override):
    from wavernn_amd.tacotron import TacotronInference
    sd = dict(_state_dict(variant))
    sd.update(override)
    if double:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return TacotronInference(sd, device=dev)


@functools.lru_cache(maxsize=None)
def _device_tts(variant='plain'):
    return _tts(torch.device('cuda', 0), variant)


def _ids(n):
    return [int(i) for i in np.random.RandomState(5).randint(0, 148, size=100)[:n]]


def _mel(N):
    return torch.randn(1, 80, 200, generator=torch.Generator().manual_seed(7))[:, :, :N].contiguous()


def _encode_torch(tts, ids):
    """(pre_rnn, seq, seq_proj) of the mirror's ops on tts's device and dtype."""
    import torch.nn.functional as F
    x = torch.as_tensor(ids, dtype=torch.long, device=tts.device).unsqueeze(0)
    x = tts._prenet(F.embedding(x, tts.p['encoder.embedding.weight']), 'encoder.pre_net').transpose(1, 2)
    pre = tts._cbhg_front(x, 'encoder.cbhg', tts._enc_k)[0]
    seq, proj = tts.encode(ids)
    return dict(pre_rnn=pre, seq=seq[0], seq_proj=proj[0])


def _postnet_torch(tts, mel):
    import torch.nn.functional as F
    m = mel.to(tts.device, tts.p['post_proj.weight'].dtype)
    pre = tts._cbhg_front(m, 'postnet', tts._post_k)[0]
    return dict(pre_rnn=pre, linear=F.linear(tts._cbhg(m, 'postnet', tts._post_k), tts.p['post_proj.weight'])[0])


def _np64(d):
    return {k: v.detach().double().cpu().numpy() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _reference(stage, variant, n):
    """float64 mirror outputs at length n (computed once, shared, never modified)."""
    t64 = _tts('cpu', variant, double=True)
    with torch.no_grad():
        return _np64(_encode_torch(t64, _ids(n)) if stage == 'encoder' else _postnet_torch(t64, _mel(n).double()))


@functools.lru_cache(maxsize=None)
def _e_ref(stage, variant):
    """Per output: max(float32 CPU mirror, float32 torch ops on the device) error against float64 at the longest length of the set."""
    n = max(ENC_N if stage == 'encoder' else POST_N)
    ref = _reference(stage, variant, n)
    dev_tts = _device_tts(variant)
    dev_tts._bigru_kernel = True                                           # today's path under generate(kernel=True)
    out = {}
    with torch.no_grad():
        for tts in (_tts('cpu', variant), dev_tts):
            got = _np64(_encode_torch(tts, _ids(n)) if stage == 'encoder' else _postnet_torch(tts, _mel(n)))
            for k, v in got.items():
                out[k] = max(out.get(k, 0.0), float(np.abs(v - ref[k]).max()))
    return out


def _check(stage, variant, n, got):
    ref, e_ref = _reference(stage, variant, n), _e_ref(stage, variant)
    worst = 0.0
    for k, v in got.items():
        v = v.detach().double().cpu().numpy()
        assert v.shape == ref[k].shape, (k, v.shape, ref[k].shape)
        err = float(np.abs(v - ref[k]).max())
        ratio = err / e_ref[k]
        worst = max(worst, ratio)
        print(f'{stage} [{variant}] n={n} {k}: max|hip - f64| = {err:.3e}, e_ref = {e_ref[k]:.3e}, ratio = {ratio:.2f} (|x| <= {np.abs(ref[k]).max():.2f})')
        assert err <= MARGIN * e_ref[k], (k, err, e_ref[k], ratio)
    return worst


def _assert_negative_bank_values(stage, variant):
    """A condition on the INPUT, checked on the mirror: with the -0.5 bias at least a quarter of the bank values the max-pool sees at
    position 0 are negative, so max(-inf, bank[0]) and max(0, bank[0]) differ there."""
    import torch.nn.functional as F
    t = _tts('cpu', variant)
    with torch.no_grad():
        if stage == 'encoder':
            x = torch.as_tensor(_ids(100), dtype=torch.long).unsqueeze(0)
            x = t._prenet(F.embedding(x, t.p['encoder.embedding.weight']), 'encoder.pre_net').transpose(1, 2)
            prefix, K = 'encoder.cbhg', t._enc_k
        else:
            x, prefix, K = _mel(200), 'postnet', t._post_k
        bank0 = torch.cat([t._bnconv(x, f'{prefix}.conv1d_bank.{k}')[:, :, 0] for k in range(K)], dim=1)
    share = float((bank0 < 0).float().mean())
    print(f'{stage}: share of negative bank values at position 0 = {share:.2f}')
    assert share >= 0.25, share


@pytest.mark.parametrize('n', ENC_N)
@pytest.mark.parametrize('variant', VARIANTS)
def test_encoder_through_wrnn_taco_encode(variant, n):
    """Embedding -> pre-net -> encoder CBHG -> GRU -> encoder_proj through `wrnn_taco_encode`: the highway output in front of the GRU
    (`pre_rnn_out`), `seq` and `seq_proj` within 8 x e_ref of the float64 mirror at every length."""
    if variant == 'negative_bank':
        _assert_negative_bank_values('encoder', variant)
    tts = _device_tts(variant)
    seq, proj, pre = tts.encode_kernel(_ids(n), want_pre_rnn=True)
    torch.cuda.synchronize()
    assert seq.shape == (1, n, 256) and proj.shape == (1, n, 256) and pre.shape == (n, 128)
    _check('encoder', variant, n, dict(pre_rnn=pre, seq=seq[0], seq_proj=proj[0]))


@pytest.mark.parametrize('N', POST_N)
@pytest.mark.parametrize('variant', VARIANTS)
def test_postnet_through_wrnn_taco_postnet(variant, N):
    """Post-net CBHG (input [n_mels][N], 8 widths, 256 / 80 projections, pre_highway) -> GRU -> post_proj through `wrnn_taco_postnet`."""
    if variant == 'negative_bank':
        _assert_negative_bank_values('postnet', variant)
    tts = _device_tts(variant)
    linear, pre = tts.postnet_kernel(_mel(N).to(tts.device), want_pre_rnn=True)
    torch.cuda.synchronize()
    assert linear.shape == (N, 80) and pre.shape == (N, 128)
    _check('postnet', variant, N, dict(pre_rnn=pre, linear=linear))


def test_pre_rnn_out_is_optional_and_changes_nothing():
    """NULL `pre_rnn_out`: not written, and the other outputs are bit-identical to a call that asks for it."""
    tts = _device_tts('plain')
    a = tts.encode_kernel(_ids(33), want_pre_rnn=True)
    b = tts.encode_kernel(_ids(33))
    p = tts.postnet_kernel(_mel(17).to(tts.device), want_pre_rnn=True)
    q = tts.postnet_kernel(_mel(17).to(tts.device))
    torch.cuda.synchronize()
    assert b[2] is None and q[1] is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(p[0], q[0])


@contextlib.contextmanager
def _deterministic_convs():
    """The torch-op path is not bit-stable from call to call by default: MIOpen's solver for `conv_project1` (2048 x 3 / 1024 x 3 terms
    per output) sums in an order that varies (measured on an MI355X on identical input: 7.5e-8 in the encoder's, 4.8e-7 in the post-net's;
    every other op, `wrnn_bigru` and the decoder kernel repeat exactly).  With `torch.backends.cudnn.deterministic` it picks a
    deterministic solver and the whole of `generate(kernel=True)` repeats bit for bit, so "the same output as before" is a bitwise
    statement under this flag only.  The HIP path uses no MIOpen op and needs no flag."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


def _golden():
    g = np.load(os.path.join(HERE, 'golden', 'tacotron_decoder_200f.npz'))
    return g['mel'], g['linear'], g['attention'], [int(i) for i in g['ids']]


def test_generate_with_cbhg_kernel_matches_the_reference():
    """End to end: ids -> `wrnn_taco_encode` -> `wrnn_taco_decode` -> `wrnn_taco_postnet` against what the REFERENCE's
    `Tacotron.generate` returned for these weights and this sentence (tests/golden/tacotron_decoder_200f.npz): mel, attention and
    linear within TACO_TOL, the bound these outputs have on the torch-op path."""
    from wavernn_amd.tacotron import text_to_ids
    ref_mel, ref_lin, ref_attn, ref_ids = _golden()
    ids = text_to_ids(IDS_TEXT)
    assert ids == ref_ids
    tts = _device_tts('plain')
    mel, lin, attn = tts.generate(ids, steps=ref_mel.shape[1], kernel=True, kernel_variant=2, cbhg_kernel=True)
    assert tts.last_front_path == 'hip'
    assert mel.shape == ref_mel.shape and lin.shape == ref_lin.shape and attn.shape == ref_attn.shape
    d = [float(np.abs(a - b).max()) for a, b in ((mel, ref_mel), (attn, ref_attn), (lin, ref_lin))]
    print('generate(cbhg_kernel=True) vs the reference: max |d| mel %.2e attention %.2e linear %.2e' % tuple(d))
    assert max(d) <= TACO_TOL, d


def test_generate_with_cbhg_kernel_repeats_and_follows_the_stream():
    """Two runs are bit-identical; a run on a non-default stream equals the run on the default stream; `cbhg_kernel=False` afterwards
    reports 'torch' and returns what it returned before the kernels were used, bit for bit (the torch ops' convolutions held to
    deterministic solvers for both of those runs: `_deterministic_convs`)."""
    from wavernn_amd.tacotron import text_to_ids
    ids = text_to_ids(IDS_TEXT)
    tts = _device_tts('plain')
    kw = dict(steps=200, kernel=True, kernel_variant=2)
    with _deterministic_convs():
        before = tts.generate(ids, **kw)
    assert tts.last_front_path == 'torch'
    a = tts.generate(ids, cbhg_kernel=True, **kw)
    b = tts.generate(ids, cbhg_kernel=True, **kw)
    assert tts.last_front_path == 'hip'
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = tts.generate(ids, cbhg_kernel=True, **kw)
    side.synchronize()
    with _deterministic_convs():
        after = tts.generate(ids, **kw)
    assert tts.last_front_path == 'torch'
    for x, y, z, u, v in zip(a, b, c, before, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)
        assert np.array_equal(u, v)


def test_unsupported_dims_stay_on_the_torch_ops():
    """An encoder whose conv_project1 has 120 channels (not a multiple of 16): `wrnn_taco_front_create` answers WRNN_ERR_ARG with a
    message, `generate(cbhg_kernel=True)` completes on the torch ops and says so; asking for the kernels directly raises."""
    from wavernn_amd import _lib
    from wavernn_amd.tacotron import text_to_ids
    sd = _state_dict('plain')
    g = torch.Generator().manual_seed(1)
    over = {'encoder.cbhg.conv_project1.conv.weight': 0.02 * torch.randn(120, 2048, 3, generator=g),
            'encoder.cbhg.conv_project2.conv.weight': 0.05 * torch.randn(128, 120, 3, generator=g)}
    for name in ('weight', 'bias', 'running_mean', 'running_var'):
        over[f'encoder.cbhg.conv_project1.bnorm.{name}'] = sd[f'encoder.cbhg.conv_project1.bnorm.{name}'][:120].clone()
    dev = torch.device('cuda', 0)
    tts = _tts(dev, **over)
    ids = text_to_ids('Hello there.')
    with _deterministic_convs():                                           # both runs are the torch ops: bitwise only under this flag
        want = tts.generate(ids, steps=12, kernel=True)
        got = tts.generate(ids, steps=12, kernel=True, cbhg_kernel=True)
    assert tts.last_front_path == 'torch' and tts._front is False
    assert 'multiples of 16' in tts._front_refused
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    with pytest.raises(_lib.WrnnError):
        tts.encode_kernel(ids)
