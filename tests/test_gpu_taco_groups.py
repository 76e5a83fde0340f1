"""Two sentence groups per launch of the batched Tacotron decoder on the GPU (-m gpu): `wrnn_taco_decode_batch_groups` /
`wrnn_taco_decode_forced_groups` (the GROUPED instantiations of wrnn_taco_batch_kernel, csrc/wrnn_taco_batch.hip: 256 workgroups, a group of up
to eight sentences on each half of the device) and `generate_batch(..., groups=2)` / `forward_gta_batch(..., groups=2)`.

The groups share the weights and nothing else, and the arithmetic is the plain kernel's, so the bar is EXACT: every sentence's mel, attention and
step count out of a grouped launch are `array_equal` to the plain `wrnn_taco_decode_batch` / `wrnn_taco_decode_forced` call on its group alone
-- whatever the other group holds, however long it runs and whichever half it sits on.  Rows past a sentence's end keep the caller's FILL, and
both workspaces' status words read clean.

Sentences, weights, threshold and helpers are those of tests/test_gpu_taco_batch.py (A 12 ids, B 74, C 224; with `stop_threshold = 0.0146` A
stops at 12 frames and B, C never do)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_gpu_taco_batch import A_TEXT, B_TEXT, C_TEXT, FILL, TACO_TOL, _enc, _status, _tts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLD = 0.0146
_MEMO = {}


def _free_call(texts, max_steps, threshold, r, weights='plain'):
    """A `wrnn_taco_batch_call` over FILLed buffers and a workspace of its own: (struct, workspace, mels, scores, steps_done, keep-alive)."""
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
    return c, ws, mels, scores, done, encs


def _free_read(call):
    """[(mel, scores, steps)] of a finished call; the status words read clean and the rows past a sentence's end still hold FILL."""
    from wavernn_amd import _lib
    c, ws, mels, scores, done, _ = call
    assert _status(_lib.lib(), ws, c.stream) == [0, 0, 0, 0]                                         # (synchronises the stream)
    out = []
    for m, a, k in zip(mels, scores, [int(k) for k in done.cpu()]):
        m, a = m.cpu().numpy(), a.cpu().numpy()
        assert 1 <= k <= m.shape[0] and np.all(m[k:] == FILL) and np.all(a[k:] == FILL), k
        out.append((m, a, k))
    return out


def _plain_free(texts, max_steps, threshold=THRESHOLD, r=1, weights='plain'):
    """The plain `wrnn_taco_decode_batch` call on one group alone: computed once per group and shared."""
    key = ('free', tuple(texts), tuple(max_steps), threshold, r, weights)
    if key not in _MEMO:
        from wavernn_amd import _lib
        call = _free_call(texts, max_steps, threshold, r, weights)
        rc = _lib.lib().wrnn_taco_decode_batch(0, ctypes.byref(_tts(r, weights).decoder_weights()), ctypes.byref(call[0]))
        assert rc == _lib.WRNN_OK, _lib.lib().wrnn_taco_last_error()
        _MEMO[key] = _free_read(call)
    return _MEMO[key]


def _grouped_free(groups, threshold=THRESHOLD, r=1, weights='plain'):
    """`wrnn_taco_decode_batch_groups` over groups = [(texts, max_steps), ...]: per group [(mel, scores, steps)]."""
    from wavernn_amd import _lib
    L = _lib.lib()
    calls = [_free_call(texts, max_steps, threshold, r, weights) for texts, max_steps in groups]
    table = (ctypes.POINTER(_lib.TacoBatchCall) * len(calls))(*[ctypes.pointer(call[0]) for call in calls])
    rc = L.wrnn_taco_decode_batch_groups(0, ctypes.byref(_tts(r, weights).decoder_weights()), table, len(calls))
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    return [_free_read(call) for call in calls]


def _assert_free_groups_equal_plain(groups, threshold=THRESHOLD, r=1, expect=None, weights='plain'):
    outs = _grouped_free(groups, threshold, r, weights)
    steps = [tuple(k for _, _, k in out) for out in outs]
    print('steps_done', steps)
    if expect is not None:
        assert steps == [tuple(e) for e in expect], steps
    for g, ((texts, max_steps), out) in enumerate(zip(groups, outs)):
        for s, ((mel, sc, k), (mel1, sc1, k1)) in enumerate(zip(out, _plain_free(texts, max_steps, threshold, r, weights))):
            print(f'group {g} sentence {s}: {k} steps, max |grouped - plain| mel {np.abs(mel[:k] - mel1[:k]).max():.3e} '
                  f'attention {np.abs(sc[:k] - sc1[:k]).max():.3e}')
            assert k == k1, (g, s, k, k1)
            assert np.array_equal(mel, mel1) and np.array_equal(sc, sc1), (g, s)                     # (the FILL rows included)
    return outs


def test_free_running_groups_of_mixed_sizes():
    """Group 0 = [A, C], group 1 = [B], 40 steps: the <2> instantiation, A ending on its stop test at 12 while its group and the other run on."""
    _assert_free_groups_equal_plain([([A_TEXT, C_TEXT], (40, 40)), ([B_TEXT], (40,))], expect=[(12, 40), (40,)])


@pytest.mark.parametrize('swap', [False, True])
def test_groups_whose_ends_are_far_apart(swap):
    """[A] for 3 steps beside [B, C, A, B, C] for 40: the <8> instantiation with one group's workgroups gone for 37 steps of the other -- and the
    same with the groups on the other halves."""
    groups = [([A_TEXT], (3,)), ([B_TEXT, C_TEXT, A_TEXT, B_TEXT, C_TEXT], (40,) * 5)]
    expect = [(3,), (40, 40, 12, 40, 40)]
    if swap:
        groups, expect = groups[::-1], expect[::-1]
    _assert_free_groups_equal_plain(groups, expect=expect)


def test_groups_at_two_frames_per_step():
    """decoder.r = 2, one pair, 20 steps = 40 frames."""
    outs = _assert_free_groups_equal_plain([([A_TEXT, B_TEXT], (20, 20)), ([C_TEXT], (20,))], threshold=_tts(2).stop_threshold, r=2,
                                           expect=[(20, 20), (20,)])
    assert outs[0][0][0].shape == (20, 80, 2)


def test_one_group_through_the_groups_entry_is_the_plain_call():
    out, = _assert_free_groups_equal_plain([([A_TEXT, B_TEXT, C_TEXT], (40, 25, 40))], expect=[(12, 25, 40)])
    assert len(out) == 3


def test_a_group_beside_another_matches_the_reference_output():
    """The sentence of tests/golden/tacotron_decoder_200f.npz as group 1 beside an unrelated group 0, 200 steps, default threshold: within the
    suite's TACO_TOL of what the REFERENCE's `Tacotron.generate` returned, as tests/test_gpu_config3.py holds the single kernel."""
    from wavernn_amd.tacotron import text_to_ids
    g = np.load(os.path.join(HERE, 'golden', 'tacotron_decoder_200f.npz'))
    assert [int(i) for i in g['ids']] == text_to_ids(B_TEXT)
    outs = _grouped_free([([A_TEXT, C_TEXT], (200, 200)), ([B_TEXT], (200,))], threshold=_tts().stop_threshold)
    mel, sc, k = outs[1][0]
    assert k == 200 and [k0 for _, _, k0 in outs[0]] == [200, 200]
    d, da = np.abs(g['mel'] - mel[:, :, 0].T).max(), np.abs(g['attention'] - sc).max()
    print(f'group 1 of a grouped launch vs the reference over 200 frames: mel {d:.3e} attention {da:.3e}')
    assert d <= TACO_TOL and da <= TACO_TOL, (d, da)


# ---- the forced form ----
PAD = 3                                                                  # rows of FILL behind every output: the caller's, never written


def _seeded_mel(N):
    from wavernn_amd.synthetic import random_mel
    return (random_mel(500 + N, N) * 8 - 4).astype(np.float32)           # [-4, 4], the decoder's scale


def _forced_call(texts, Ns, r, weights='plain', mels=None):
    """A `wrnn_taco_forced_call` over FILLed buffers and a workspace of its own; the forced mels are `_seeded_mel(N)`, or `mels` ((80, N) each)."""
    from wavernn_amd import _lib
    L, tts, dev = _lib.lib(), _tts(r, weights), torch.device('cuda', 0)
    S = len(texts)
    encs = [_enc(t, r, weights) for t in texts]
    force = [torch.from_numpy(np.ascontiguousarray(m, np.float32)).to(dev) for m in (mels or [_seeded_mel(N) for N in Ns])]
    assert [f.shape for f in force] == [(80, N) for N in Ns]
    steps = [(N + r - 1) // r for N in Ns]
    outs = [torch.full((k + PAD, 80, r), FILL, device=dev) for k in steps]
    scores = [torch.full((k + PAD, e[0].size(0)), FILL, device=dev) for k, e in zip(steps, encs)]
    frames = (ctypes.c_int32 * S)(*Ns)
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
    return c, ws, outs, scores, steps, (encs, force)


def _forced_read(call):
    from wavernn_amd import _lib
    c, ws, outs, scores, steps, _ = call
    assert _status(_lib.lib(), ws, c.stream) == [0, 0, 0, 0]
    res = []
    for m, a, k in zip(outs, scores, steps):
        m, a = m.cpu().numpy(), a.cpu().numpy()
        assert np.all(m[k:] == FILL) and np.all(a[k:] == FILL)           # rows past the sentence's own steps keep their fill value
        np.testing.assert_allclose(a[:k].sum(axis=1), 1.0, atol=1e-5)
        res.append((m, a))
    return res


@pytest.mark.parametrize('r', [1, 2])
def test_forced_groups(r):
    """Group 0 = one sentence of ONE frame (a single step), group 1 = [B / 37, C / 5, A / 24] (at r = 2: frame counts r does not divide): each
    sentence against `wrnn_taco_decode_forced` on its group alone."""
    from wavernn_amd import _lib
    L, w = _lib.lib(), _tts(r).decoder_weights()
    groups = [([A_TEXT], [1]), ([B_TEXT, C_TEXT, A_TEXT], [37, 5, 24])]
    plain = []
    for texts, Ns in groups:
        call = _forced_call(texts, Ns, r)
        rc = L.wrnn_taco_decode_forced(0, ctypes.byref(w), ctypes.byref(call[0]))
        assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
        plain.append(_forced_read(call))
    calls = [_forced_call(texts, Ns, r) for texts, Ns in groups]
    table = (ctypes.POINTER(_lib.TacoForcedCall) * 2)(*[ctypes.pointer(call[0]) for call in calls])
    rc = L.wrnn_taco_decode_forced_groups(0, ctypes.byref(w), table, 2)
    assert rc == _lib.WRNN_OK, L.wrnn_taco_last_error()
    for g, (call, ref) in enumerate(zip(calls, plain)):
        assert call[4] == [(N + r - 1) // r for N in groups[g][1]]
        for s, ((m, a), (m1, a1)) in enumerate(zip(_forced_read(call), ref)):
            print(f'r = {r} group {g} sentence {s}: {call[4][s]} steps, max |grouped - plain| mel {np.abs(m - m1).max():.3e} attention {np.abs(a - a1).max():.3e}')
            assert np.array_equal(m, m1) and np.array_equal(a, a1), (g, s)
    # one group through the new entry is the plain call
    call = _forced_call(*groups[1], r)
    table1 = (ctypes.POINTER(_lib.TacoForcedCall) * 1)(ctypes.pointer(call[0]))
    assert L.wrnn_taco_decode_forced_groups(0, ctypes.byref(w), table1, 1) == _lib.WRNN_OK, L.wrnn_taco_last_error()
    for (m, a), (m1, a1) in zip(_forced_read(call), plain[1]):
        assert np.array_equal(m, m1) and np.array_equal(a, a1)


# ---- Python ----
def _eleven():
    from wavernn_amd.tacotron import text_to_ids
    texts = [A_TEXT, B_TEXT, B_TEXT[:30], 'Hi.', B_TEXT[:51], A_TEXT + ' ' + A_TEXT, B_TEXT[10:], B_TEXT[:17], C_TEXT[:120], B_TEXT[5:40], A_TEXT[:7]]
    return [text_to_ids(t) for t in texts]


def test_generate_batch_with_two_groups_equals_one_group():
    """11 sentences, max_batch = 4: groups = 2 decodes one pair of groups of four in a grouped launch and the group of three by the plain call."""
    tts, ids = _tts(), _eleven()
    one = tts.generate_batch(ids, steps=16, cbhg_kernel=True, max_batch=4)
    assert tts.last_decode_groups == [(4,), (4,), (3,)]
    two = tts.generate_batch(ids, steps=16, cbhg_kernel=True, max_batch=4, groups=2)
    assert tts.last_decode_groups == [(4, 4), (3,)]
    assert len(one) == len(two) == 11
    for u, (o, t) in enumerate(zip(one, two)):
        assert all(np.array_equal(x, y) for x, y in zip(o, t)) and o[0].shape == (80, 16), u


def test_forward_gta_batch_with_two_groups_equals_one_group():
    tts, ids = _tts(), _eleven()
    Ns = [31, 5, 40, 9, 23, 12, 37, 16, 5, 28, 3]
    mels = [_seeded_mel(N) for N in Ns]
    one = tts.forward_gta_batch(ids, mels, cbhg_kernel=True, max_batch=4)
    assert tts.last_decode_groups == [(4,), (4,), (3,)]
    two = tts.forward_gta_batch(ids, mels, cbhg_kernel=True, max_batch=4, groups=2)
    assert tts.last_decode_groups == [(4, 4), (3,)]
    for u, (N, o, t) in enumerate(zip(Ns, one, two)):
        assert all(np.array_equal(x, y) for x, y in zip(o, t)) and o[0].shape == (80, N), u
