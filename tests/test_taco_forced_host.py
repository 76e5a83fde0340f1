"""The host side of the ground-truth-aligned path, without a GPU: the C ABI of `wrnn_taco_decode_forced` (symbols, header, argument checks that
return before a device is needed), the workspace size, the grouping of `TacotronInference.forward_gta_batch` (with a fake decode function) and
the `python -m wavernn_amd.gta_tacotron --no_kernel` command line on a two-utterance dataset."""
import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

FAKE = 0x1000                                                            # a non-null "device pointer": the checks under test never follow it


def _lib_or_build():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    _lib, L = _lib_or_build()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read(), flags=re.S)
    for sym in ('wrnn_taco_forced_workspace_bytes', 'wrnn_taco_decode_forced'):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and re.search(r'\b%s\s*\(' % sym, hdr), sym
    assert 'typedef struct wrnn_taco_forced_call' in hdr
    assert L.wrnn_abi_version() == 9 == _lib.ABI_VERSION and re.search(r'#define\s+WRNN_ABI_VERSION\s+9\b', hdr)
    # the ctypes struct lays out as the C struct does: 4 x 32 bit, 7 pointers, a pointer, a size, a pointer
    assert ctypes.sizeof(_lib.TacoForcedCall) == 16 + 10 * ctypes.sizeof(ctypes.c_void_p)


def _weights(_lib):
    w = _lib.TacoWeights()
    w.struct_bytes = ctypes.sizeof(_lib.TacoWeights)
    w.n_mels, w.prenet1, w.prenet2, w.decoder_dims, w.encoder_width, w.lstm_dims, w.attn_filters, w.attn_kernel = 80, 256, 128, 256, 256, 512, 32, 31
    for name in _lib.TACO_WEIGHT_FIELDS:
        setattr(w, name, FAKE)
    return w


def _call(_lib, L, n=(74, 12, 224), frames=(40, 23, 16), r=1, max_r=2):
    S = len(n)
    c = _lib.TacoForcedCall()
    c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
    c.n_sent, c.r, c.max_r = S, r, max_r
    c.n, c.frames = (ctypes.c_int32 * S)(*n), (ctypes.c_int32 * S)(*frames)
    for name in ('seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * S)(*([FAKE] * S)))
    c.workspace = FAKE
    c.workspace_bytes = L.wrnn_taco_forced_workspace_bytes(S, c.frames, r)
    return c


def _refused(_lib, L, c, w=None):
    rc = L.wrnn_taco_decode_forced(0, ctypes.byref(w if w is not None else _weights(_lib)), ctypes.byref(c))
    assert rc == _lib.ERR_ARG, rc
    return L.wrnn_taco_last_error().decode()


def test_every_argument_error_returns_before_a_device_is_needed():
    _lib, L = _lib_or_build()
    assert L.wrnn_taco_decode_forced(0, None, None) == _lib.ERR_ARG
    c = _call(_lib, L)
    c.struct_bytes -= 4
    assert 'struct size' in _refused(_lib, L, c)
    for S in (0, 9):
        c = _call(_lib, L)
        c.n_sent = S
        assert f'n_sent={S}' in _refused(_lib, L, c)
    for r, max_r in ((0, 2), (3, 2), (9, 16)):
        c = _call(_lib, L, r=1, max_r=max_r)
        c.r = r
        assert f'r={r}' in _refused(_lib, L, c)
    for table in ('n', 'frames', 'seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'):
        c = _call(_lib, L)
        setattr(c, table, None)
        assert 'null buffer' in _refused(_lib, L, c), table
    c = _call(_lib, L)
    c.workspace = None
    assert 'null buffer' in _refused(_lib, L, c)
    # per sentence: the message names it
    for bad in (0, 257):
        msg = _refused(_lib, L, _call(_lib, L, n=(74, bad, 224)))
        assert 'sentence 1' in msg and f'n={bad}' in msg and '256' in msg, msg
    for bad in (0, -5, (1 << 20) + 1):
        c = _call(_lib, L)
        c.frames[2] = bad
        msg = _refused(_lib, L, c)
        assert 'sentence 2' in msg and f'frames={bad}' in msg and str(1 << 20) in msg, msg
    for name in ('seq', 'seq_proj', 'force_mel', 'mel_out', 'scores_out'):
        c = _call(_lib, L)
        getattr(c, name)[1] = None
        msg = _refused(_lib, L, c)
        assert 'sentence 1' in msg and 'null buffer' in msg, (name, msg)
    c = _call(_lib, L)
    c.workspace_bytes -= 1
    msg = _refused(_lib, L, c)
    assert 'workspace' in msg and str(c.workspace_bytes + 1) in msg, msg
    w = _weights(_lib)
    w.lstm_dims = 256
    assert 'geometry' in _refused(_lib, L, _call(_lib, L), w)
    # the limits themselves are accepted by the checks: 2^20 frames, 256 positions, r = max_r = 8 (the call then asks for a device: not here)
    c = _call(_lib, L, n=(256,), frames=(1 << 20,), r=8, max_r=8)
    assert c.workspace_bytes > 0


def test_workspace_bytes():
    _lib, L = _lib_or_build()
    ws = lambda frames, r=1, S=None: int(L.wrnn_taco_forced_workspace_bytes(len(frames) if S is None else S, (ctypes.c_int32 * len(frames))(*frames), r))
    assert ws((40,)) > int(L.wrnn_taco_batch_workspace_bytes(1)) and ws((40,)) - int(L.wrnn_taco_batch_workspace_bytes(1)) == 40 * 128 * 4
    # grows with the SUM of steps, 512 bytes per step, on top of the batched decoder's workspace for that many sentences
    assert ws((40, 23, 16)) - int(L.wrnn_taco_batch_workspace_bytes(3)) == (40 + 23 + 16) * 512
    assert ws((41, 23, 16)) - ws((40, 23, 16)) == 512
    assert ws((37, 23), r=2) - int(L.wrnn_taco_batch_workspace_bytes(2)) == (19 + 12) * 512
    assert ws((1 << 20,) * 8) - int(L.wrnn_taco_batch_workspace_bytes(8)) == 8 * (1 << 20) * 512
    # bad tables
    assert ws((40, 0)) == 0 and ws((40, -1)) == 0 and ws((40, (1 << 20) + 1)) == 0
    assert ws((40,), r=0) == 0 and ws((40,), r=9) == 0
    assert ws((40,), S=0) == 0 and ws((40,) * 9) == 0
    assert int(L.wrnn_taco_forced_workspace_bytes(1, None, 1)) == 0


def _seed3():
    from wavernn_amd.synthetic import random_tacotron_state_dict
    return random_tacotron_state_dict(3, json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json'))))


def test_forward_gta_batch_groups_by_steps_and_restores_the_callers_order():
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    assert TacotronInference._gta_groups([5, 2, 9, 2, 7], 2) == [[1, 3], [0, 4], [2]]           # a stable sort by steps, groups of <= 2
    tts = TacotronInference(_seed3())
    tts.encode = lambda ids: (torch.zeros(1, len(ids), 256), torch.zeros(1, len(ids), 256))    # (the encoder is not what is checked)
    calls = []

    def fake_decode(encs, mels):
        """marks every output with its sentence's frame count"""
        calls.append([m.size(1) for m in mels])
        assert all(m.dtype == torch.float32 and m.is_contiguous() and m.size(0) == 80 for m in mels)
        return [(torch.full((1, 80, m.size(1)), float(m.size(1))), torch.full((m.size(1), e[0].size(1)), float(m.size(1)))) for e, m in zip(encs, mels)]
    tts._decode_forced_kernel = fake_decode
    Ns = [31, 5, 40, 9, 23, 12, 37, 16, 5, 28, 3]
    ids = [text_to_ids('ab' * (k + 1)) for k in range(len(Ns))]
    mels = [np.zeros((80, N), np.float32) for N in Ns]
    outs = tts.forward_gta_batch(ids, mels, kernel=True, max_batch=4)
    assert calls == [[3, 5, 5, 9], [12, 16, 23, 28], [31, 37, 40]]
    assert all(len(c) <= 4 for c in calls) and sorted(sum(calls, [])) == sorted(Ns)
    for N, i, (gta, lin, attn) in zip(Ns, ids, outs):                    # the caller's order
        assert gta.shape == (80, N) and lin.shape == (80, N) and attn.shape == (N, len(i)) and np.all(gta == N) and np.all(attn == N)
    calls.clear()
    tts.forward_gta_batch(ids, mels, kernel=True, max_batch=8)
    assert [len(c) for c in calls] == [8, 3] and sum(calls, []) == sorted(Ns)
    with pytest.raises(ValueError):
        tts.forward_gta_batch(ids, mels, kernel=True, max_batch=9)
    with pytest.raises(ValueError):
        tts.forward_gta_batch(ids, mels[:-1])


def test_the_kernel_path_does_not_fall_back_to_the_host():
    from wavernn_amd import _lib
    from wavernn_amd.tacotron import TacotronInference
    tts = TacotronInference(_seed3())
    assert tts.device.type == 'cpu'
    with pytest.raises(_lib.WrnnError):
        tts.forward_gta([3, 4, 5], np.zeros((80, 4), np.float32), kernel=True)
    with pytest.raises(_lib.WrnnError):
        tts.forward_gta_batch([[3, 4, 5]], [np.zeros((80, 4), np.float32)])


def test_cli_no_kernel_writes_the_references_file_set(tmp_path, monkeypatch):
    from wavernn_amd import gta_tacotron
    from wavernn_amd.synthetic import random_mel
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)       # the eager path on the CPU, also where a GPU is present
    sd = _seed3()
    torch.save(sd, tmp_path / 'tts.pyt')
    data = tmp_path / 'data'
    (data / 'mel').mkdir(parents=True)
    texts = {'LJ001-0001': 'Hello there.', 'LJ001-0002': 'Printing, in the only sense.'}
    dataset = [('LJ001-0001', 7), ('LJ001-0002', 4)]
    for u, (item_id, N) in enumerate(dataset):
        np.save(data / 'mel' / f'{item_id}.npy', random_mel(40 + u, N))
    pickle.dump(dataset, open(data / 'dataset.pkl', 'wb'))
    pickle.dump(texts, open(data / 'text_dict.pkl', 'wb'))
    gta_tacotron.main(['--tts_weights', str(tmp_path / 'tts.pyt'), '--path', str(data), '--no_kernel'])
    assert sorted(p.name for p in (data / 'gta').iterdir()) == ['LJ001-0001.npy', 'LJ001-0002.npy']
    tts = TacotronInference(sd)
    for u, (item_id, N) in enumerate(dataset):
        got = np.load(data / 'gta' / f'{item_id}.npy')
        assert got.shape == (80, N) and got.dtype == np.float32
        _, lin, _ = tts.forward_gta(text_to_ids(texts[item_id]), random_mel(40 + u, N) * 8 - 4)          # `_, gta, _ = model(x, mels)`
        assert np.array_equal(got, ((lin[:, :N] + 4) / 8).astype(np.float32))
    # --out, and the kernel path refuses to run without a device instead of falling back
    gta_tacotron.main(['--tts_weights', str(tmp_path / 'tts.pyt'), '--path', str(data), '--no_kernel', '--out', str(tmp_path / 'elsewhere')])
    assert sorted(p.name for p in (tmp_path / 'elsewhere').iterdir()) == ['LJ001-0001.npy', 'LJ001-0002.npy']
    with pytest.raises(SystemExit):
        gta_tacotron.main(['--tts_weights', str(tmp_path / 'tts.pyt'), '--path', str(data)])
