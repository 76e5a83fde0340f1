"""The teacher-forced Tacotron decoder on the GPU (-m gpu): `wrnn_taco_decode_forced` (the PreNet pre-pass wrnn_taco_prenet_kernel and the
FORCED instantiations of wrnn_taco_batch_kernel, csrc/wrnn_taco_batch.hip) and `TacotronInference.forward_gta` / `forward_gta_batch`.

Bars: against the REFERENCE's own `Tacotron.forward(x, m, generate_gta=True)` (tests/golden/tacotron_gta.npz, scripts/make_golden_gta.py) the
suite's TACO_TOL = 1e-6 -- the bound tests/test_gpu_config3.py holds the free-running kernels to over 200 compounding frames; teacher forcing
compounds less.  Against the same sentence decoded alone, and against the free-running kernel fed its own output back: `array_equal` -- the
arithmetic is the same and contraction is off.  The reference is 0.48 .. 0.58 away from the free-running output for these weights, so a kernel
that ignored the forced mel cannot pass.

Sentences, weights and helpers are those of tests/test_gpu_taco_batch.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_gpu_taco_batch import A_TEXT, B_TEXT, C_TEXT, FILL, TACO_TOL, _batch, _enc, _status, _tts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 3                                                                  # rows of FILL behind every output: the caller's, never written
_G = {}


def _golden():
    if 'g' not in _G:
        _G['g'] = np.load(os.path.join(HERE, 'golden', 'tacotron_gta.npz'))
    return _G['g']


def _case(tag, text, r):
    from wavernn_amd.tacotron import text_to_ids
    g = _golden()
    assert [int(i) for i in g[f'{tag}_ids']] == text_to_ids(text) and int(g[f'{tag}_r']) == r
    return g[f'{tag}_force_mel'], g[f'{tag}_gta'], g[f'{tag}_attention']


def _seeded_mel(N):
    from wavernn_amd.synthetic import random_mel
    return (random_mel(500 + N, N) * 8 - 4).astype(np.float32)


def _forced(texts, mels, r=1, weights='plain'):
    """`wrnn_taco_decode_forced` into FILLed buffers of steps_s + PAD rows: [(mel (80, steps_s r), attention (steps_s, n_s))] per sentence.  The
    status words must read clean and the PAD rows must still hold FILL."""
    from wavernn_amd import _lib
    L, tts, dev = _lib.lib(), _tts(r, weights), torch.device('cuda', 0)
    S = len(texts)
    encs = [_enc(t, r, weights) for t in texts]
    force = [torch.from_numpy(np.ascontiguousarray(m, np.float32)).to(dev) for m in mels]
    steps = [(m.shape[1] + r - 1) // r for m in mels]
    outs = [torch.full((k + PAD, 80, r), FILL, device=dev) for k in steps]
    scores = [torch.full((k + PAD, e[0].size(0)), FILL, device=dev) for k, e in zip(steps, encs)]
    frames = (ctypes.c_int32 * S)(*[m.shape[1] for m in mels])
    need = int(L.wrnn_taco_forced_workspace_bytes(S, frames, r))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    c = _lib.TacoForcedCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
    c.n_sent, c.r, c.max_r = S, r, tts.max_r
    c.n = (ctypes.c_int32 * S)(*[e[0].size(0) for e in encs])
    c.frames = frames
    for name, ts in (('seq', [e[0] for e in encs]), ('seq_proj', [e[1] for e in encs]), ('force_mel', force), ('mel_out', outs), ('scores_out', scores)):
        setattr(c, name, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts]))
    c.workspace, c.workspace_bytes = ws.data_ptr(), ws.numel()
    c.stream = torch.cuda.current_stream(dev).cuda_stream
    rc = L.wrnn_taco_decode_forced(0, ctypes.byref(tts.decoder_weights()), ctypes.byref(c))
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    assert _status(L, ws, c.stream) == [0, 0, 0, 0]                      # (synchronises the stream)
    res = []
    for m, a, k in zip(outs, scores, steps):
        m, a = m.cpu().numpy(), a.cpu().numpy()
        assert np.all(m[k:] == FILL) and np.all(a[k:] == FILL)           # rows past the sentence's own steps keep their fill value
        np.testing.assert_allclose(a[:k].sum(axis=1), 1.0, atol=1e-5)
        res.append((np.ascontiguousarray(m[:k].transpose(1, 0, 2)).reshape(80, k * r), a[:k]))
    return res


def _alone(text, mel, r=1):
    key = ('alone', text, mel.shape[1], r)
    if key not in _G:
        _G[key] = _forced([text], [mel], r)[0]
    return _G[key]


def _assert_reference(tag, got, ref_gta, ref_attn):
    d, da = float(np.abs(got[0] - ref_gta).max()), float(np.abs(got[1] - ref_attn).max())
    print(f'{tag}: forced kernel vs the reference: mel {d:.3e} attention {da:.3e}')
    assert got[0].shape == ref_gta.shape and got[1].shape == ref_attn.shape
    assert d <= TACO_TOL and da <= TACO_TOL, (tag, d, da)


def test_group_of_three_matches_the_reference():
    """[B / 40, A / 23, C / 16]: the <4, true> instantiation, ragged ends, C's 224 positions on the rows past 128."""
    cases = [_case('g0', B_TEXT, 1), _case('g1', A_TEXT, 1), _case('g2', C_TEXT, 1)]
    outs = _forced([B_TEXT, A_TEXT, C_TEXT], [c[0] for c in cases])
    for tag, got, c in zip(('B/40', 'A/23', 'C/16'), outs, cases):
        _assert_reference(tag, got, c[1], c[2])


def test_one_sentence_matches_the_reference():
    """B alone: the <2, true> instantiation."""
    force, gta, attn = _case('g0', B_TEXT, 1)
    _assert_reference('B/40 alone', _alone(B_TEXT, force), gta, attn)


def test_two_frames_per_step_with_an_odd_length_matches_the_reference():
    """[B, A] at r = 2 with N = (37, 23): 19 and 12 steps, 38 and 24 frames out; B against the reference, A against A alone."""
    force, gta, attn = _case('g3', B_TEXT, 2)
    mel_a = _seeded_mel(23)
    outs = _forced([B_TEXT, A_TEXT], [force, mel_a], r=2)
    assert outs[0][0].shape == (80, 38) and outs[0][1].shape == (19, 74) and outs[1][0].shape == (80, 24) and outs[1][1].shape == (12, 12)
    _assert_reference('B/37 r=2', outs[0], gta, attn)
    alone = _alone(A_TEXT, mel_a, r=2)
    assert np.array_equal(outs[1][0], alone[0]) and np.array_equal(outs[1][1], alone[1])


def test_eight_sentences_do_not_depend_on_their_company():
    """The <8, true> (LEAN) instantiation: every sentence out of the group of eight is `array_equal` to the same sentence decoded alone."""
    texts = [A_TEXT, B_TEXT, C_TEXT, B_TEXT[:30], B_TEXT + ' ' + A_TEXT, B_TEXT + ' ' + B_TEXT, 'Hi.', C_TEXT + ' ' + A_TEXT]
    Ns = (5, 9, 12, 16, 23, 31, 37, 40)
    mels = [_seeded_mel(N) for N in Ns]
    outs = _forced(texts, mels)
    for text, mel, (m, a) in zip(texts, mels, outs):
        m1, a1 = _alone(text, mel)
        print(f'{len(text):4d} chars, N = {mel.shape[1]}: max |group - alone| mel {np.abs(m - m1).max():.3e} attention {np.abs(a - a1).max():.3e}')
        assert m.shape == (80, mel.shape[1]) and np.array_equal(m, m1) and np.array_equal(a, a1), text[:20]


@pytest.mark.parametrize('r', [1, 2])
def test_forced_on_the_free_running_output_is_the_free_running_output(r):
    """B free-running for 24 steps (`wrnn_taco_decode_batch`, a threshold no frame is below), its mel fed back as the forced mel: the PreNet
    pre-pass then sees what L1 / L2 of the loop saw, and the forced mel and attention must be the free-running ones bit for bit."""
    mel, sc, k = _batch([B_TEXT], (24,), -1e9, r)[0]
    assert k == 24
    free = np.ascontiguousarray(mel.transpose(1, 0, 2)).reshape(80, 24 * r)
    got = _alone(B_TEXT, free, r)
    print(f'r = {r}: max |forced - free-running| mel {np.abs(got[0] - free).max():.3e} attention {np.abs(got[1] - sc).max():.3e}')
    assert np.array_equal(got[0], free) and np.array_equal(got[1], sc)


def test_a_single_step_reads_only_the_go_frame():
    """A / 1: one step, one frame; the output equals the fixture and nothing else is written (the PAD rows are checked in `_forced`)."""
    force, gta, attn = _case('g4', A_TEXT, 1)
    assert force.shape == (80, 1)
    got = _alone(A_TEXT, force)
    assert got[0].shape == (80, 1) and got[1].shape == (1, 12)
    _assert_reference('A/1', got, gta, attn)
    other = _forced([A_TEXT], [force + 1.0])[0]                          # the only frame is never read: <GO> feeds the only step
    assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1])


def test_forward_gta_batch_equals_forward_gta_per_sentence():
    from wavernn_amd.tacotron import text_to_ids
    g, tts = _golden(), _tts()
    ids = [text_to_ids(B_TEXT), text_to_ids(A_TEXT)]
    mels = [g['g0_force_mel'], g['g1_force_mel']]
    outs = tts.forward_gta_batch(ids, mels, cbhg_kernel=True)
    assert tts.last_front_path == 'hip' and [o[0].shape for o in outs] == [(80, 40), (80, 23)]
    for u, tag in enumerate(('g0', 'g1')):
        one = tts.forward_gta(ids[u], mels[u], kernel=True, cbhg_kernel=True)
        assert all(np.array_equal(x, y) for x, y in zip(outs[u], one)), tag
        d = float(np.abs(outs[u][1] - g[f'{tag}_linear']).max())
        print(f'{tag}: linear vs the reference {d:.3e}, gta {np.abs(outs[u][0] - g[f"{tag}_gta"]).max():.3e}')
        assert outs[u][1].shape == g[f'{tag}_linear'].shape and d <= TACO_TOL, (tag, d)
    again = tts.forward_gta_batch(ids, mels, cbhg_kernel=True, max_batch=1)
    assert all(np.array_equal(x, y) for o, p in zip(outs, again) for x, y in zip(o, p))
