"""The encoder and the post-net for a LIST of sentences in one call (-m gpu): `wrnn_taco_encode_many`, `wrnn_taco_postnet_many`,
`wrnn_bigru_many` (csrc/wrnn_cbhg.hip, csrc/wrnn_taco.hip) and `TacotronInference.generate_batch(cbhg_kernel=True)` on top of them.

The `_many` kernels run the tile bodies of the single-sentence kernels with sentence-relative positions, so the bar is EXACT everywhere:
`torch.equal` against the single-sentence entry point on that sentence alone (which tests/test_gpu_cbhg.py holds to its float64 yardstick).
No tolerance is introduced here.  Weights: those of tests/test_gpu_cbhg.py in its four variants -- with 'negative_bank' a max-pool that
looked at the previous sentence's last row instead of -inf changes position 0 of every sentence but the first, with 'random_bnorm' a wrong
scale / shift base does, and with 'rich' (every bias vector random too) so does a bias read at another sentence's offset.

Every output buffer is allocated PAD rows longer than the call needs and filled with FILL; the workspace gets GUARD bytes behind the queried
size.  The rows behind the last sentence and the guard must read back unchanged."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_cbhg import IDS_TEXT, VARIANTS, _device_tts, _ids, _mel

pytestmark = pytest.mark.gpu
FILL, PAD, GUARD, GUARD_BYTE = 7.5, 8, 4096, 0xA5
ENC_LENGTHS = (17, 1, 16, 33)            # several tiles, one position, exactly a tile, a tile plus one: every boundary falls mid-tile in the row space
POST_LENGTHS = (1, 17, 48)
_MEMO = {}


def _split(seq, lengths):
    out, o = [], 0
    for k in lengths:
        out.append(seq[o:o + k])
        o += k
    assert o == len(seq)
    return out


def _enc_sentences(lengths=ENC_LENGTHS):
    """Distinct sentences: consecutive slices of the suite's 100 random ids."""
    return [tuple(s) for s in _split(_ids(sum(lengths)), lengths)]


def _post_mels(lengths=POST_LENGTHS):
    """Distinct [80][N_s] inputs on the device: consecutive column ranges of the suite's random mel, each its own contiguous tensor."""
    m = _mel(sum(lengths))[0]
    cols = _split(list(range(sum(lengths))), lengths)
    return [m[:, c[0]:c[-1] + 1].contiguous().to(torch.device('cuda', 0)) for c in cols]


def _workspace(L, tts, n, k):
    need = int(L.wrnn_taco_front_workspace_bytes_many(tts._front_handle(), n, k))
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=tts.device)
    assert ws.data_ptr() % 256 == 0
    return ws, need


def _check_untouched(ws, need, rows, *bufs):
    assert bool((ws[need:] == GUARD_BYTE).all()), 'the guard bytes behind the workspace were written'
    for b in bufs:
        if b is not None:
            assert bool((b[rows:] == FILL).all()), 'rows behind the last sentence were written'


def _encode_many(tts, sentences, want_pre=True):
    """`wrnn_taco_encode_many` into FILLed, oversized buffers: per sentence dict(seq, seq_proj[, pre_rnn]) (clones)."""
    from wavernn_amd import _lib
    L, dev, k = _lib.lib(), tts.device, len(sentences)
    lengths = [len(s) for s in sentences]
    rows = sum(lengths)
    n = (ctypes.c_int32 * k)(*lengths)
    ws, need = _workspace(L, tts, n, k)
    ids = torch.tensor([i for s in sentences for i in s], dtype=torch.int32).to(dev)
    seq, proj = torch.full((rows + PAD, 256), FILL, device=dev), torch.full((rows + PAD, 256), FILL, device=dev)
    pre = torch.full((rows + PAD, 128), FILL, device=dev) if want_pre else None
    rc = L.wrnn_taco_encode_many(tts._front_handle(), ids.data_ptr(), n, k, seq.data_ptr(), proj.data_ptr(), pre.data_ptr() if want_pre else None,
                                 ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    torch.cuda.current_stream(dev).synchronize()
    _check_untouched(ws, need, rows, seq, proj, pre)
    out = []
    for a, b, c in zip(_split(seq[:rows], lengths), _split(proj[:rows], lengths), _split(pre[:rows], lengths) if want_pre else [None] * k):
        out.append(dict(seq=a.clone(), seq_proj=b.clone(), **(dict(pre_rnn=c.clone()) if want_pre else {})))
    return out


def _postnet_many(tts, mels, want_pre=True):
    """`wrnn_taco_postnet_many` into FILLed, oversized buffers: per sentence dict(linear[, pre_rnn]) (clones)."""
    from wavernn_amd import _lib
    L, dev, k = _lib.lib(), tts.device, len(mels)
    lengths = [m.size(1) for m in mels]
    rows = sum(lengths)
    n = (ctypes.c_int32 * k)(*lengths)
    ws, need = _workspace(L, tts, n, k)
    ptrs = (ctypes.c_void_p * k)(*[m.data_ptr() for m in mels])
    linear = torch.full((rows + PAD, 80), FILL, device=dev)
    pre = torch.full((rows + PAD, 128), FILL, device=dev) if want_pre else None
    rc = L.wrnn_taco_postnet_many(tts._front_handle(), ptrs, n, k, linear.data_ptr(), pre.data_ptr() if want_pre else None, ws.data_ptr(), need,
                                  torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    torch.cuda.current_stream(dev).synchronize()
    _check_untouched(ws, need, rows, linear, pre)
    out = []
    for a, c in zip(_split(linear[:rows], lengths), _split(pre[:rows], lengths) if want_pre else [None] * k):
        out.append(dict(linear=a.clone(), **(dict(pre_rnn=c.clone()) if want_pre else {})))
    return out


def _encode_alone(variant, sentence):
    """`encode_kernel` (wrnn_taco_encode) of one sentence: computed once per (variant, sentence), shared, never modified."""
    key = ('enc', variant, sentence)
    if key not in _MEMO:
        seq, proj, pre = _device_tts(variant).encode_kernel(list(sentence), want_pre_rnn=True)
        torch.cuda.synchronize()
        _MEMO[key] = dict(seq=seq[0], seq_proj=proj[0], pre_rnn=pre)
    return _MEMO[key]


def _postnet_alone(variant, index, mel):
    key = ('post', variant, index, mel.size(1))
    if key not in _MEMO:
        linear, pre = _device_tts(variant).postnet_kernel(mel, want_pre_rnn=True)
        torch.cuda.synchronize()
        _MEMO[key] = dict(linear=linear, pre_rnn=pre)
    return _MEMO[key]


def _assert_same_bits(got, want, what):
    for k, v in got.items():
        assert v.shape == want[k].shape, (what, k, v.shape, want[k].shape)
        d = float((v - want[k]).abs().max())
        print(f'{what} {k}: max |many - alone| = {d:.3e}')
        assert torch.equal(v, want[k]), (what, k, d)


@pytest.mark.parametrize('variant', VARIANTS)
def test_encoder_sentences_equal_the_single_call(variant):
    """(17, 1, 16, 33) ids in one call: `seq`, `seq_proj` and `pre_rnn_out` of every sentence are the bits of `wrnn_taco_encode` alone; the same
    four sentences in reversed order give the same per-sentence bits."""
    tts, sents = _device_tts(variant), _enc_sentences()
    got = _encode_many(tts, sents)
    for s, g in zip(sents, got):
        assert g['seq'].shape == (len(s), 256) and g['pre_rnn'].shape == (len(s), 128)
        _assert_same_bits(g, _encode_alone(variant, s), f'encoder [{variant}] n={len(s)}')
    back = _encode_many(tts, sents[::-1])[::-1]
    for s, g, b in zip(sents, got, back):
        _assert_same_bits(b, g, f'encoder [{variant}] reversed n={len(s)}')


@pytest.mark.parametrize('variant', VARIANTS)
def test_postnet_sentences_equal_the_single_call(variant):
    """(1, 17, 48) frames from their own [n_mels][N] tensors: `linear` and `pre_rnn_out` are the bits of `wrnn_taco_postnet` alone."""
    tts, mels = _device_tts(variant), _post_mels()
    got = _postnet_many(tts, mels)
    for i, (m, g) in enumerate(zip(mels, got)):
        assert g['linear'].shape == (m.size(1), 80)
        _assert_same_bits(g, _postnet_alone(variant, i, m), f'postnet [{variant}] N={m.size(1)}')
    back = _postnet_many(tts, mels[::-1])[::-1]
    for m, g, b in zip(mels, got, back):
        _assert_same_bits(b, g, f'postnet [{variant}] reversed N={m.size(1)}')


def test_bigru_many_equals_three_bigru_calls():
    """T = (1, 2, 19), random gi, the post-net's GRU weights: out of `wrnn_bigru_many` equals three `wrnn_bigru` calls on the slices."""
    _bigru_many_equals_bigru_calls('plain')


def test_bigru_many_equals_three_bigru_calls_with_a_recurrent_bias():
    """The same on the 'rich' weights: b_hh of both directions random in +-0.1 (zero in the plain weights)."""
    p = _device_tts('rich').p
    assert float(p['postnet.rnn.bias_hh_l0'].abs().max()) > 0.05 and float(p['postnet.rnn.bias_hh_l0_reverse'].abs().max()) > 0.05
    _bigru_many_equals_bigru_calls('rich')


def _bigru_many_equals_bigru_calls(variant):
    from wavernn_amd import _lib
    L, tts = _lib.lib(), _device_tts(variant)
    dev, T = tts.device, (1, 2, 19)
    rows = sum(T)
    g = torch.Generator().manual_seed(17)
    gi = [torch.randn(rows, 384, generator=g).to(dev) for _ in range(2)]
    w = [tts.p['postnet.rnn.' + n].to(dev, torch.float32).contiguous() for n in ('weight_hh_l0', 'weight_hh_l0_reverse', 'bias_hh_l0', 'bias_hh_l0_reverse')]
    stream = torch.cuda.current_stream(dev).cuda_stream
    many = torch.full((rows + PAD, 256), FILL, device=dev)
    c = _lib.BigruManyCall()
    c.struct_bytes, c.n_seq, c.hidden, c.T = ctypes.sizeof(_lib.BigruManyCall), len(T), 128, (ctypes.c_int32 * len(T))(*T)
    c.gi_fwd, c.gi_rev, c.w_hh_fwd, c.w_hh_rev, c.b_hh_fwd, c.b_hh_rev = [t.data_ptr() for t in gi + w]
    c.out, c.stream = many.data_ptr(), stream
    assert L.wrnn_bigru_many(0, ctypes.byref(c)) == _lib.WRNN_OK, L.wrnn_taco_last_error()
    alone = torch.full((rows + PAD, 256), FILL, device=dev)
    o = 0
    for t in T:
        b = _lib.BigruCall()
        b.struct_bytes, b.T, b.hidden = ctypes.sizeof(_lib.BigruCall), t, 128
        b.gi_fwd, b.gi_rev = gi[0].data_ptr() + o * 384 * 4, gi[1].data_ptr() + o * 384 * 4
        b.w_hh_fwd, b.w_hh_rev, b.b_hh_fwd, b.b_hh_rev = [x.data_ptr() for x in w]
        b.out, b.stream = alone.data_ptr() + o * 256 * 4, stream
        assert L.wrnn_bigru(0, ctypes.byref(b)) == _lib.WRNN_OK, L.wrnn_taco_last_error()
        o += t
    torch.cuda.synchronize()
    assert bool((many[rows:] == FILL).all()) and bool((alone[rows:] == FILL).all())
    assert float(many[:rows].abs().max()) > 0 and bool((many[:rows] != FILL).all())
    assert torch.equal(many, alone)


def test_pre_rnn_out_null_changes_nothing_else():
    tts = _device_tts('plain')
    sents, mels = _enc_sentences(), _post_mels()
    for a, b in zip(_encode_many(tts, sents), _encode_many(tts, sents, want_pre=False)):
        assert set(b) == {'seq', 'seq_proj'} and torch.equal(a['seq'], b['seq']) and torch.equal(a['seq_proj'], b['seq_proj'])
    for a, b in zip(_postnet_many(tts, mels), _postnet_many(tts, mels, want_pre=False)):
        assert set(b) == {'linear'} and torch.equal(a['linear'], b['linear'])


def test_call_on_a_side_stream_equals_the_default_stream():
    tts = _device_tts('plain')
    sents, mels = _enc_sentences(), _post_mels()
    enc, post = _encode_many(tts, sents), _postnet_many(tts, mels)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc_s, post_s = _encode_many(tts, sents), _postnet_many(tts, mels)
    side.synchronize()
    for a, b in zip(enc + post, enc_s + post_s):
        _assert_same_bits(b, a, 'side stream')


def test_full_width_64_sentences():
    """64 sentences of lengths 1..64 (2080 rows) per call: sentences 0, 31 and 63 against the single-sentence calls."""
    tts = _device_tts('negative_bank')
    lengths = list(range(1, 65))
    rs = np.random.RandomState(9)
    sents = [tuple(int(i) for i in rs.randint(0, 148, size=k)) for k in lengths]
    got = _encode_many(tts, sents)
    mel = torch.randn(80, sum(lengths), generator=torch.Generator().manual_seed(8))
    mels = [mel[:, sum(lengths[:i]):sum(lengths[:i + 1])].contiguous().to(tts.device) for i in range(64)]
    post = _postnet_many(tts, mels)
    for i in (0, 31, 63):
        _assert_same_bits(got[i], _encode_alone('negative_bank', sents[i]), f'encoder sentence {i}')
        _assert_same_bits(post[i], _postnet_alone('negative_bank', 100 + i, mels[i]), f'postnet sentence {i}')


def test_python_many_methods_return_per_sentence_views():
    """`encode_kernel_many` / `postnet_kernel_many`: per-sentence views in the shapes of `encode_kernel` / `postnet_kernel`, the same bits."""
    tts, sents, mels = _device_tts('random_bnorm'), _enc_sentences(), _post_mels()
    enc = tts.encode_kernel_many([list(s) for s in sents], want_pre_rnn=True)
    post = tts.postnet_kernel_many([m.unsqueeze(0) for m in mels], want_pre_rnn=True)
    plain = tts.encode_kernel_many([list(s) for s in sents])
    torch.cuda.synchronize()
    assert len(enc) == len(sents) and len(post) == len(mels) and all(e[2] is None for e in plain)
    for s, (seq, proj, pre) in zip(sents, enc):
        assert seq.shape == (1, len(s), 256) and proj.shape == (1, len(s), 256) and pre.shape == (len(s), 128)
        assert seq[0].is_contiguous() and seq.data_ptr() % 16 == 0 and proj.data_ptr() % 16 == 0
        _assert_same_bits(dict(seq=seq[0], seq_proj=proj[0], pre_rnn=pre), _encode_alone('random_bnorm', s), 'encode_kernel_many')
    for i, (m, (linear, pre)) in enumerate(zip(mels, post)):
        _assert_same_bits(dict(linear=linear, pre_rnn=pre), _postnet_alone('random_bnorm', i, m), 'postnet_kernel_many')
    with pytest.raises(ValueError):
        tts.encode_kernel_many([[1, 2]] * 65)
    with pytest.raises(ValueError):
        tts.encode_kernel_many([[1, 2], []])


@pytest.mark.parametrize('max_batch', [8, 1])
def test_generate_batch_equals_generate_per_sentence(max_batch):
    """`generate_batch([A, B, C], steps=24, cbhg_kernel=True)` (12, 74 and 224 ids): mel, linear and attention of every sentence `array_equal`
    to `generate(ids, steps=24, kernel=True, cbhg_kernel=True)`; the same with one sentence per decoder kernel."""
    from wavernn_amd.tacotron import text_to_ids
    tts = _device_tts('plain')
    sents = [text_to_ids(t) for t in ('Hello there.', IDS_TEXT, ' '.join([IDS_TEXT] * 3))]
    assert [len(s) for s in sents] == [12, 74, 224]
    if 'alone' not in _MEMO:
        _MEMO['alone'] = [tts.generate(ids, steps=24, kernel=True, cbhg_kernel=True) for ids in sents]
        assert tts.last_front_path == 'hip'
    tts.last_front_path = None
    outs = tts.generate_batch(sents, steps=24, cbhg_kernel=True, max_batch=max_batch)
    assert tts.last_front_path == 'hip' and len(outs) == 3
    for ids, got, want in zip(sents, outs, _MEMO['alone']):
        assert [g.shape for g in got] == [w.shape for w in want] == [(80, 24), (80, 24), (24, len(ids))]
        for name, g, w in zip(('mel', 'linear', 'attention'), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (len(ids), name, float(np.abs(g - w).max()))
    one, = tts.generate_batch(sents[1:2], steps=24, cbhg_kernel=True, max_batch=max_batch)      # a list of one: the single-sentence entry points
    assert tts.last_front_path == 'hip' and all(np.array_equal(g, w) for g, w in zip(one, _MEMO['alone'][1]))
