"""wrnn_taco_batch_kernel on the GPU (-m gpu): up to eight sentences per pass of the Tacotron decoder kernel (csrc/wrnn_taco_batch.hip,
`wrnn_taco_decode_batch`, `TacotronInference.generate_batch`).  The batched kernel sums every row in the order of the single-sentence
register-resident kernel, so the bar is EXACT: a sentence's mel block, attention and step count out of a batch are `array_equal` to
`wrnn_taco_decode(variant=2)` of that sentence alone -- whatever rides along and wherever the others end.

Sentences: A = 'Hello there.' (12 ids), B = the suite's CERN sentence (74 ids), C = B three times (224 ids).  For the suite's weights the CPU
mirror's per-frame mel maxima over frames 8-39 are A 0.014406 .. 0.014453, B 0.014718 .. 0.014790, C 0.014859 .. 0.014933: with
`stop_threshold = 0.0146` A stops at the first t > 10 (12 frames) and B, C never do -- margin >= 1.1e-4 on both sides against a
kernel-versus-mirror difference of 7.5e-9."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 7.5                                                               # what the caller's output buffers hold before a decode
TACO_TOL = 1e-6                                                          # the suite's bound against the reference's own output (test_gpu_config3.py)
A_TEXT = 'Hello there.'
B_TEXT = 'Scientists at the CERN laboratory say they have discovered a new particle.'
C_TEXT = ' '.join([B_TEXT] * 3)
_MEMO = {}


def _tts(r=1, weights='plain'):
    """The suite's weights on the device; weights='rich': `helpers.rich_tacotron_state_dict(5)`, every bias and batch norm random
    (tests/test_gpu_taco_rich.py)."""
    if ('tts', r, weights) not in _MEMO:
        from helpers import rich_tacotron_state_dict
        from wavernn_amd.synthetic import random_tacotron_state_dict
        from wavernn_amd.tacotron import TacotronInference
        shapes = json.load(open(os.path.join(HERE, 'golden', 'tacotron_shapes.json')))
        sd = rich_tacotron_state_dict(5, shapes) if weights == 'rich' else random_tacotron_state_dict(3, shapes)
        if r != 1:
            sd['decoder.r' if 'decoder.r' in sd else 'r'] = torch.tensor(r)
        tts = TacotronInference(sd, device=torch.device('cuda', 0))
        assert tts.r == r
        _MEMO['tts', r, weights] = tts
    return _MEMO['tts', r, weights]


def _enc(text, r=1, weights='plain'):
    """(seq, seq_proj) of a sentence, [n][256] each, computed once."""
    if ('enc', text, r, weights) not in _MEMO:
        from wavernn_amd.tacotron import text_to_ids
        tts = _tts(r, weights)
        with torch.no_grad():
            seq, proj = tts.encode(text_to_ids(text))
        _MEMO['enc', text, r, weights] = (seq[0].contiguous(), proj[0].contiguous())
    return _MEMO['enc', text, r, weights]


def _status(L, ws, stream):
    from wavernn_amd import _lib
    st4 = (ctypes.c_uint32 * 4)()
    assert L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), stream) == _lib.WRNN_OK
    return list(st4)


def _single(text, max_steps, threshold, r=1, weights='plain'):
    """`wrnn_taco_decode(variant=2)` of one sentence into FILLed buffers: (mel [max_steps][80][r], scores [max_steps][n], steps).  Computed once
    per (sentence, limit, threshold, r, weights) and shared."""
    key = ('single', text, max_steps, threshold, r, weights)
    if key not in _MEMO:
        from wavernn_amd import _lib
        L, tts, dev = _lib.lib(), _tts(r, weights), torch.device('cuda', 0)
        seq, proj = _enc(text, r, weights)
        n = seq.size(0)
        mel = torch.full((max_steps, 80, r), FILL, device=dev)
        scores = torch.full((max_steps, n), FILL, device=dev)
        done = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(L.wrnn_taco_workspace_bytes()), dtype=torch.uint8, device=dev)
        c = _lib.TacoCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoCall)
        c.n, c.r, c.max_r, c.max_steps, c.stop_threshold, c.variant = n, r, tts.max_r, max_steps, threshold, 2
        c.seq, c.seq_proj, c.mel_out, c.scores_out = seq.data_ptr(), proj.data_ptr(), mel.data_ptr(), scores.data_ptr()
        c.steps_done, c.workspace, c.workspace_bytes = done.data_ptr(), ws.data_ptr(), ws.numel()
        c.stream = torch.cuda.current_stream(dev).cuda_stream
        rc = L.wrnn_taco_decode(0, ctypes.byref(tts.decoder_weights()), ctypes.byref(c))
        assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
        assert _status(L, ws, c.stream) == [0, 0, 0, 0]
        _MEMO[key] = (mel.cpu().numpy(), scores.cpu().numpy(), int(done.item()))
    return _MEMO[key]


def _batch(texts, max_steps, threshold, r=1, weights='plain'):
    """`wrnn_taco_decode_batch` into FILLed buffers: [(mel, scores, steps)] per sentence; the status words must read clean."""
    from wavernn_amd import _lib
    L, tts, dev = _lib.lib(), _tts(r, weights), torch.device('cuda', 0)
    S = len(texts)
    encs = [_enc(t, r, weights) for t in texts]
    mels = [torch.full((m, 80, r), FILL, device=dev) for m in max_steps]
    scores = [torch.full((m, e[0].size(0)), FILL, device=dev) for m, e in zip(max_steps, encs)]
    done = torch.full((S,), -1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.wrnn_taco_batch_workspace_bytes(S)), dtype=torch.uint8, device=dev)
    c = _lib.TacoBatchCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
    c.n_sent, c.r, c.max_r, c.stop_threshold = S, r, tts.max_r, threshold
    c.n = (ctypes.c_int32 * S)(*[e[0].size(0) for e in encs])
    c.max_steps = (ctypes.c_int32 * S)(*max_steps)
    for name, ts in (('seq', [e[0] for e in encs]), ('seq_proj', [e[1] for e in encs]), ('mel_out', mels), ('scores_out', scores)):
        setattr(c, name, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts]))
    c.steps_done, c.workspace, c.workspace_bytes = done.data_ptr(), ws.data_ptr(), ws.numel()
    c.stream = torch.cuda.current_stream(dev).cuda_stream
    rc = L.wrnn_taco_decode_batch(0, ctypes.byref(tts.decoder_weights()), ctypes.byref(c))
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    assert _status(L, ws, c.stream) == [0, 0, 0, 0]                                                  # (synchronises the stream)
    ks = [int(k) for k in done.cpu()]
    return [(m.cpu().numpy(), a.cpu().numpy(), k) for m, a, k in zip(mels, scores, ks)]


def _assert_equal_to_single(texts, max_steps, threshold, r=1, expect=None, weights='plain'):
    outs = _batch(texts, max_steps, threshold, r, weights)
    steps = tuple(k for _, _, k in outs)
    print('steps_done', steps)
    if expect is not None:
        assert steps == tuple(expect), steps
    for text, limit, (mel, sc, k) in zip(texts, max_steps, outs):
        mel1, sc1, k1 = _single(text, limit, threshold, r, weights)
        assert k == k1, (text[:20], k, k1)
        print(f'{len(text):4d} chars: {k} steps, max |batch - single| mel {np.abs(mel[:k] - mel1[:k]).max():.3e} attention {np.abs(sc[:k] - sc1[:k]).max():.3e}')
        assert np.array_equal(mel[:k], mel1[:k]), text[:20]
        assert np.array_equal(sc[:k], sc1[:k]), text[:20]
        assert np.all(mel[k:] == FILL) and np.all(sc[k:] == FILL), text[:20]        # rows past the sentence's end are the caller's
        np.testing.assert_allclose(sc[:k].sum(axis=1), 1.0, atol=1e-5)
    return outs


def test_batch_is_bitwise_the_single_kernel_with_mixed_ends():
    """[A, B, C], threshold 0.0146, limits (40, 25, 40): A ends on its stop test at 12, B on its limit at 25, C on its limit at 40."""
    _assert_equal_to_single([A_TEXT, B_TEXT, C_TEXT], (40, 25, 40), 0.0146, expect=(12, 25, 40))


def test_all_sentences_stop_early_and_the_kernel_returns():
    """Threshold 1e9: every frame is below it, every sentence ends at the first t > 10."""
    _assert_equal_to_single([A_TEXT, B_TEXT, C_TEXT], (40, 25, 40), 1e9, expect=(12, 12, 12))


def test_two_frames_per_step():
    """decoder.r = 2: the `[:, :, :r]` view of mel_proj (:262), 20 steps = 40 frames."""
    outs = _assert_equal_to_single([A_TEXT, B_TEXT], (20, 20), _tts(2).stop_threshold, r=2, expect=(20, 20))
    assert outs[0][0].shape == (20, 80, 2)


def test_full_width_eight_sentences():
    texts = [A_TEXT, B_TEXT, C_TEXT, B_TEXT[:30], B_TEXT + ' ' + A_TEXT, B_TEXT + ' ' + B_TEXT, 'Hi.', C_TEXT + ' ' + A_TEXT]
    from wavernn_amd.tacotron import text_to_ids
    lens = [len(text_to_ids(t)) for t in texts]
    assert len(set(lens)) == 8 and max(lens) <= 256 and lens[:3] == [12, 74, 224], lens
    _assert_equal_to_single(texts, (16,) * 8, _tts().stop_threshold, expect=(16,) * 8)


def test_one_sentence_through_the_batch_entry():
    _assert_equal_to_single([B_TEXT], (25,), 0.0146, expect=(25,))


def test_batch_matches_the_reference_output():
    """[B, A] at 200 steps, default threshold: B's mel and attention against what the REFERENCE's `Tacotron.generate` returned for these weights
    (tests/golden/tacotron_decoder_200f.npz), within the suite's TACO_TOL."""
    from wavernn_amd.tacotron import text_to_ids
    g = np.load(os.path.join(HERE, 'golden', 'tacotron_decoder_200f.npz'))
    assert [int(i) for i in g['ids']] == text_to_ids(B_TEXT)
    (mel, sc, k), (_, _, ka) = _batch([B_TEXT, A_TEXT], (200, 200), _tts().stop_threshold)
    assert (k, ka) == (200, 200)
    d, da = np.abs(g['mel'] - mel[:, :, 0].T).max(), np.abs(g['attention'] - sc).max()
    print(f'batched kernel vs the reference over 200 frames: mel {d:.3e} attention {da:.3e}')
    assert d <= TACO_TOL and da <= TACO_TOL, (d, da)


def test_generate_batch_then_one_vocoder_pass_equals_per_sentence_synthesis(tmp_path):
    """`generate_batch([A, B], cbhg_kernel=True)` + `generate_corpus(noise_source='library', seeds=[5, 6])` against `generate(kernel=True,
    cbhg_kernel=True)` + `voc.generate` with noise_source = 'library' and noise_seed = 5 / 6: equal waveforms (what generate_corpus documents)."""
    from wavernn_amd.batch import generate_corpus
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, SHIPPED
    from wavernn_amd.tacotron import text_to_ids, tacotron_to_wavernn_mel
    tts = _tts()
    voc = WaveRNN(**SHIPPED, mode='MOL')
    voc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(0, mode='MOL').items()}, strict=True)
    voc = voc.to(torch.device('cuda', 0))
    sents, seeds = [text_to_ids(A_TEXT), text_to_ids(B_TEXT)], [5, 6]
    outs = tts.generate_batch(sents, steps=24, cbhg_kernel=True)
    assert tts.last_front_path == 'hip' and [o[0].shape for o in outs] == [(80, 24), (80, 24)]
    assert tts._batch_ws is not None and tts.decoder_weights() is tts.decoder_weights()
    mels = [torch.tensor(tacotron_to_wavernn_mel(lin)).unsqueeze(0) for _, lin, _ in outs]
    wavs = generate_corpus(voc, mels, 550, 55, True, seeds=seeds, noise_source='library')
    voc.noise_source = 'library'
    for u, ids in enumerate(sents):
        mel1, lin1, attn1 = tts.generate(ids, steps=24, kernel=True, cbhg_kernel=True)
        assert np.array_equal(outs[u][0], mel1) and np.array_equal(outs[u][1], lin1) and np.array_equal(outs[u][2], attn1), u
        voc.noise_seed = seeds[u]
        alone = voc.generate(torch.tensor(tacotron_to_wavernn_mel(lin1)).unsqueeze(0), tmp_path / f'{u}.wav', True, 550, 55, True)
        assert alone.shape == wavs[u].shape == (23 * 275,) and np.array_equal(alone, wavs[u]), u
    # a group size below the sentence count: two kernels, the same results
    again = tts.generate_batch(sents, steps=24, cbhg_kernel=True, max_batch=1)
    assert all(np.array_equal(x, y) for o, p in zip(outs, again) for x, y in zip(o, p))
