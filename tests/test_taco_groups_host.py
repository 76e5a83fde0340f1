"""The host side of two sentence groups per launch, without a GPU: the C ABI of `wrnn_taco_decode_batch_groups` /
`wrnn_taco_decode_forced_groups` (symbols, header, every refusal issued before a device is needed, the delegation of n_groups = 1), the grouped
kernel's block -> (group, workgroup) map, and the pairing of decoder groups in `TacotronInference.generate_batch` / `forward_gta_batch`
(with fake decode functions)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

FAKE = 0x10000                                                           # a non-null "device pointer": the checks under test never follow it
WS0, WS1 = 0x10000000, 0x20000000                                        # two "workspaces" far apart


def _lib_or_build():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    _lib, L = _lib_or_build()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read(), flags=re.S)
    for sym in ('wrnn_taco_decode_batch_groups', 'wrnn_taco_decode_forced_groups', 'wrnn_debug_taco_group_of'):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and re.search(r'\b%s\s*\(' % sym, hdr), sym
    assert re.search(r'#define\s+WRNN_TACO_GROUPS_MAX\s+2\b', hdr) and _lib.TACO_GROUPS_MAX == 2
    assert L.wrnn_abi_version() == 9 == _lib.ABI_VERSION and re.search(r'#define\s+WRNN_ABI_VERSION\s+9\b', hdr)


def _weights(_lib):
    w = _lib.TacoWeights()
    w.struct_bytes = ctypes.sizeof(_lib.TacoWeights)
    w.n_mels, w.prenet1, w.prenet2, w.decoder_dims, w.encoder_width, w.lstm_dims, w.attn_filters, w.attn_kernel = 80, 256, 128, 256, 256, 512, 32, 31
    for name in _lib.TACO_WEIGHT_FIELDS:
        setattr(w, name, FAKE)
    return w


def _free(_lib, L, n=(74, 12), workspace=WS0, r=1, max_r=2):
    S = len(n)
    c = _lib.TacoBatchCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
    c.n_sent, c.r, c.max_r, c.stop_threshold = S, r, max_r, -3.4
    c.n, c.max_steps = (ctypes.c_int32 * S)(*n), (ctypes.c_int32 * S)(*([40] * S))
    for name in ('seq', 'seq_proj', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * S)(*([FAKE] * S)))
    c.steps_done, c.workspace = FAKE, workspace
    c.workspace_bytes = L.wrnn_taco_batch_workspace_bytes(S)
    return c


def _forced(_lib, L, n=(74, 12), frames=(40, 23), workspace=WS0, r=1, max_r=2):
    S = len(n)
    c = _lib.TacoForcedCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
    c.n_sent, c.r, c.max_r = S, r, max_r
    c.n, c.frames = (ctypes.c_int32 * S)(*n), (ctypes.c_int32 * S)(*frames)
    for name in ('seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * S)(*([FAKE] * S)))
    c.workspace = workspace
    c.workspace_bytes = L.wrnn_taco_forced_workspace_bytes(S, c.frames, r)
    return c


FORMS = [('wrnn_taco_decode_batch_groups', 'wrnn_taco_decode_batch', 'TacoBatchCall', _free),
         ('wrnn_taco_decode_forced_groups', 'wrnn_taco_decode_forced', 'TacoForcedCall', _forced)]


def _run(_lib, L, entry, struct, calls, n_groups=None, w=None):
    table = (ctypes.POINTER(getattr(_lib, struct)) * len(calls))(*[ctypes.pointer(c) if c is not None else None for c in calls])
    rc = getattr(L, entry)(0, ctypes.byref(w if w is not None else _weights(_lib)), table, len(calls) if n_groups is None else n_groups)
    return rc, L.wrnn_taco_last_error().decode()


def _refused(*a, **kw):
    rc, msg = _run(*a, **kw)
    assert rc == -1, (rc, msg)                                           # WRNN_ERR_ARG
    return msg


@pytest.mark.parametrize('entry,plain,struct,make', FORMS)
def test_every_refusal_is_issued_before_a_device_is_needed(entry, plain, struct, make):
    _lib, L = _lib_or_build()
    assert _lib.ERR_ARG == -1
    pair = lambda **kw: [make(_lib, L, workspace=WS0), make(_lib, L, n=(224, 30), workspace=WS1, **kw)]
    # the count and the table
    for n_groups in (0, -1, 3):
        msg = _refused(_lib, L, entry, struct, pair(), n_groups=n_groups)
        assert f'n_groups={n_groups}' in msg and '1..2' in msg and 'WRNN_TACO_GROUPS_MAX' in msg, msg
    assert getattr(L, entry)(0, ctypes.byref(_weights(_lib)), None, 2) == _lib.ERR_ARG and 'calls' in L.wrnn_taco_last_error().decode()
    msg = _refused(_lib, L, entry, struct, [make(_lib, L), None])
    assert 'group 1' in msg and 'null' in msg, msg
    msg = _refused(_lib, L, entry, struct, [None, make(_lib, L)])
    assert 'group 0' in msg and 'null' in msg, msg
    # the plain call's checks, per group, with the group in front
    calls = pair()
    calls[1].n[1] = 257
    msg = _refused(_lib, L, entry, struct, calls)
    assert msg.startswith('group 1: sentence 1') and 'n=257' in msg and '256' in msg, msg
    calls = pair()
    calls[0].n_sent = 9
    assert _refused(_lib, L, entry, struct, calls).startswith('group 0: n_sent=9')
    calls = pair()
    calls[1].workspace_bytes -= 1
    msg = _refused(_lib, L, entry, struct, calls)
    assert msg.startswith('group 1: workspace') and str(calls[1].workspace_bytes + 1) in msg, msg
    calls = pair()
    calls[1].mel_out[0] = None
    msg = _refused(_lib, L, entry, struct, calls)
    assert msg.startswith('group 1: sentence 0') and 'null buffer' in msg, msg
    calls = pair()
    calls[0].struct_bytes -= 4
    assert _refused(_lib, L, entry, struct, calls).startswith('group 0: struct size')
    w = _weights(_lib)
    w.lstm_dims = 256
    assert 'geometry' in _refused(_lib, L, entry, struct, pair(), w=w)
    # what the groups of a launch must share
    calls = pair()
    calls[1].stream = 0x40
    msg = _refused(_lib, L, entry, struct, calls)
    assert 'stream' in msg and 'one stream' in msg, msg
    msg = _refused(_lib, L, entry, struct, [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS1, r=2, max_r=2)])
    assert 'r=2' in msg and 'r=1' in msg and 'equal' in msg, msg
    msg = _refused(_lib, L, entry, struct, [make(_lib, L, workspace=WS0, r=1, max_r=2), make(_lib, L, workspace=WS1, r=1, max_r=3)])
    assert 'max_r=3' in msg and 'max_r=2' in msg, msg
    # ... and what they must not: overlapping workspaces (the same one, one byte of overlap at either end); adjacent ranges are fine
    size = make(_lib, L).workspace_bytes
    for ws1 in (WS0, WS0 + size - 1, WS0 - size + 1):
        msg = _refused(_lib, L, entry, struct, [make(_lib, L, workspace=WS0), make(_lib, L, workspace=ws1)])
        assert 'overlap' in msg and 'workspace' in msg, msg
    # valid arguments (adjacent workspaces included) get as far as the plain call does on this machine: the same code
    want = getattr(L, plain)(0, ctypes.byref(_weights(_lib)), ctypes.byref(make(_lib, L)))
    if not torch.cuda.is_available():
        assert want != _lib.WRNN_OK and want != _lib.ERR_ARG
        assert _run(_lib, L, entry, struct, pair())[0] == want
        assert _run(_lib, L, entry, struct, [make(_lib, L, workspace=WS0), make(_lib, L, workspace=WS0 + size)])[0] == want
        assert _run(_lib, L, entry, struct, [make(_lib, L)])[0] == want   # n_groups = 1: the plain call itself
    # n_groups = 1 delegates: the plain call's message, without a group in front
    c = make(_lib, L)
    c.n[0] = 0
    msg = _refused(_lib, L, entry, struct, [c])
    assert msg.startswith('sentence 0') and 'n=0' in msg, msg


def test_the_block_map_is_a_bijection_onto_two_groups_of_128():
    _lib, L = _lib_or_build()
    seen, placement = set(), None
    for block in range(256):
        g, l = ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = L.wrnn_debug_taco_group_of(block, ctypes.byref(g), ctypes.byref(l))
        assert rc in (0, 1) and (placement is None or rc == placement)
        placement = rc
        assert 0 <= g.value < 2 and 0 <= l.value < 128, (block, g.value, l.value)
        seen.add((g.value, l.value))
        want = (block // 128, block % 128) if placement == 0 else ((block % 8) // 4, (block // 8) * 4 + block % 4)
        assert (g.value, l.value) == want, (block, placement)
    assert len(seen) == 256
    g, l = ctypes.c_int32(7), ctypes.c_int32(7)
    for block in (-1, 256):
        assert L.wrnn_debug_taco_group_of(block, ctypes.byref(g), ctypes.byref(l)) == -1 and (g.value, l.value) == (7, 7)
    assert L.wrnn_debug_taco_group_of(0, None, ctypes.byref(l)) == -1


# ---- the pairing of decoder groups in Python ----
def test_pair_groups():
    from wavernn_amd.tacotron import TacotronInference
    pair = TacotronInference._pair_groups
    G = [[0, 1], [2, 3], [4, 5], [6, 7], [8]]
    assert pair([], 1) == [] and pair([], 2) == []
    assert pair(G[:1], 2) == [[[0, 1]]] and pair(G[:1], 1) == [[[0, 1]]]
    assert pair(G[:2], 2) == [[[0, 1], [2, 3]]] and pair(G[:2], 1) == [[[0, 1]], [[2, 3]]]
    assert pair(G[:3], 2) == [[[0, 1], [2, 3]], [[4, 5]]]                 # an odd one out, alone
    assert pair(G, 2) == [[[0, 1], [2, 3]], [[4, 5], [6, 7]], [[8]]]
    assert pair(G, 1) == [[g] for g in G]
    for bad in (0, 3, -1, None, 2.5, True, '2'):
        with pytest.raises(ValueError):
            pair(G, bad)


def _seed3():
    from wavernn_amd.synthetic import random_tacotron_state_dict
    return random_tacotron_state_dict(3, json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json'))))


def _fake_tts():
    """An instance whose encoder and decode functions are fakes that record what they are asked and mark every output with its sentence: the
    forced ones with the frame count, the free-running ones with the id count."""
    from wavernn_amd.tacotron import TacotronInference
    tts = TacotronInference(_seed3())
    tts.device = torch.device('cuda', 0)                                 # (never used: every device call below is a fake)
    tts.encode = lambda ids: (torch.zeros(1, len(ids), 256), torch.zeros(1, len(ids), 256))
    tts._cbhg = lambda mel, prefix, K: torch.zeros(1, mel.size(2), tts.p['post_proj.weight'].shape[1])
    calls = []
    forced = lambda encs, mels: [(torch.full((1, 80, m.size(1)), float(m.size(1))), torch.full((m.size(1), e[0].size(1)), float(m.size(1))))
                                 for e, m in zip(encs, mels)]
    free = lambda encs, steps: [(torch.full((1, 80, steps), float(e[0].size(1))), torch.full((steps, e[0].size(1)), float(e[0].size(1)))) for e in encs]

    def forced_one(encs, mels):
        calls.append(('plain', [m.size(1) for m in mels]))
        return forced(encs, mels)

    def forced_many(groups):
        calls.append(('grouped', [[m.size(1) for m in mels] for _, mels in groups]))
        return [forced(encs, mels) for encs, mels in groups]

    def free_one(encs, steps):
        calls.append(('plain', [e[0].size(1) for e in encs]))
        return free(encs, steps)

    def free_many(groups, steps):
        calls.append(('grouped', [[e[0].size(1) for e in encs] for encs in groups]))
        return [free(encs, steps) for encs in groups]
    tts._decode_forced_kernel, tts._decode_forced_launch = forced_one, forced_many
    tts._decode_batch_kernel, tts._decode_batch_launch = free_one, free_many
    return tts, calls


def test_forward_gta_batch_pairs_neighbouring_groups_and_keeps_the_callers_order(monkeypatch):
    from wavernn_amd.tacotron import text_to_ids
    tts, calls = _fake_tts()
    monkeypatch.setattr(tts, '_forced_mel', lambda mel: torch.as_tensor(np.asarray(mel)).reshape(80, -1))
    Ns = [31, 5, 40, 9, 23, 12, 37, 16, 5, 28, 3]
    ids = [text_to_ids('ab' * (k + 1)) for k in range(len(Ns))]
    mels = [np.zeros((80, N), np.float32) for N in Ns]
    outs = tts.forward_gta_batch(ids, mels, kernel=True, max_batch=4, groups=2)
    assert calls == [('grouped', [[3, 5, 5, 9], [12, 16, 23, 28]]), ('plain', [31, 37, 40])]
    for N, i, (gta, lin, attn) in zip(Ns, ids, outs):                    # the caller's order
        assert gta.shape == (80, N) and attn.shape == (N, len(i)) and np.all(gta == N) and np.all(attn == N)
    calls.clear()
    tts.forward_gta_batch(ids, mels, kernel=True, max_batch=2, groups=2)  # 6 groups (5 of two, one of one): three pairs
    assert [kind for kind, _ in calls] == ['grouped'] * 3
    assert [c[1] for c in calls] == [[[3, 5], [5, 9]], [[12, 16], [23, 28]], [[31, 37], [40]]]
    calls.clear()
    tts.forward_gta_batch(ids, mels, kernel=True, max_batch=4, groups=1)  # the default: what ran before the argument existed
    assert calls == [('plain', [3, 5, 5, 9]), ('plain', [12, 16, 23, 28]), ('plain', [31, 37, 40])]
    calls.clear()
    tts.forward_gta_batch(ids, mels, kernel=True, max_batch=4)
    assert [kind for kind, _ in calls] == ['plain'] * 3
    for bad in (0, 3):
        with pytest.raises(ValueError):
            tts.forward_gta_batch(ids, mels, kernel=True, max_batch=4, groups=bad)
    with pytest.raises(ValueError):
        tts.forward_gta_batch(ids, mels, kernel=True, max_batch=9, groups=2)   # max_batch keeps its 1..8 check


def test_generate_batch_pairs_consecutive_groups_and_keeps_the_callers_order():
    from wavernn_amd.tacotron import text_to_ids
    tts, calls = _fake_tts()
    ids = [text_to_ids('ab' * (k + 1)) for k in range(11)]               # 2, 4, .. 22 ids
    outs = tts.generate_batch(ids, steps=6, kernel=True, max_batch=4, groups=2)
    assert calls == [('grouped', [[2, 4, 6, 8], [10, 12, 14, 16]]), ('plain', [18, 20, 22])]
    for i, (mel, lin, attn) in zip(ids, outs):
        assert mel.shape == (80, 6) and attn.shape == (6, len(i)) and np.all(mel == len(i)) and np.all(attn == len(i))
    calls.clear()
    tts.generate_batch(ids, steps=6, kernel=True, max_batch=4)
    assert calls == [('plain', [2, 4, 6, 8]), ('plain', [10, 12, 14, 16]), ('plain', [18, 20, 22])]
    calls.clear()
    tts.generate_batch(ids[:5], steps=6, kernel=True, max_batch=8, groups=2)  # one group: nothing to pair
    assert calls == [('plain', [2, 4, 6, 8, 10])]
    calls.clear()
    assert tts.generate_batch([], steps=6, kernel=True, groups=2) == [] and calls == []
    for bad in (0, 3):
        with pytest.raises(ValueError):
            tts.generate_batch(ids, steps=6, kernel=True, max_batch=4, groups=bad)


def test_the_clis_take_groups():
    from wavernn_amd import gen_tacotron, gta_tacotron
    for mod in (gen_tacotron, gta_tacotron):
        src = open(mod.__file__).read()
        assert "'--groups'" in src and 'choices=[1, 2]' in src and 'groups=a.groups' in src
