"""The batched Tacotron decoder's entry points (csrc/wrnn_taco_batch.hip: `wrnn_taco_decode_batch`, `wrnn_taco_batch_workspace_bytes`) and
`TacotronInference.generate_batch` without a GPU: the header and the binding declare them, every bad argument is WRNN_ERR_ARG with a message
that names the sentence and the limit BEFORE any device is touched (so also on a host without one), and the any-device form of
`generate_batch` is the per-sentence `generate()`.  The kernel itself: tests/test_gpu_taco_batch.py."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

FAKE = 0x1000                                   # a non-null pointer that is never dereferenced before the device check


def _lib():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def _weights(_l):
    w = _l.TacoWeights()
    w.struct_bytes = ctypes.sizeof(_l.TacoWeights)
    w.n_mels, w.prenet1, w.prenet2, w.decoder_dims, w.encoder_width, w.lstm_dims, w.attn_filters, w.attn_kernel = 80, 256, 128, 256, 256, 512, 32, 31
    for n in _l.TACO_WEIGHT_FIELDS:
        setattr(w, n, FAKE)
    return w


def _call(_l, L, n=(12, 74, 224), max_steps=(40, 25, 40), r=1, max_r=20):
    """A valid wrnn_taco_batch_call over fake device pointers (kept alive by the returned struct's attributes)."""
    S = len(n)
    c = _l.TacoBatchCall()
    c.struct_bytes = ctypes.sizeof(_l.TacoBatchCall)
    c.n_sent, c.r, c.max_r, c.stop_threshold = S, r, max_r, -3.4
    c.n = (ctypes.c_int32 * S)(*n)
    c.max_steps = (ctypes.c_int32 * S)(*max_steps)
    for name in ('seq', 'seq_proj', 'mel_out', 'scores_out'):
        setattr(c, name, (ctypes.c_void_p * S)(*([FAKE] * S)))
    c.steps_done, c.workspace = FAKE, FAKE
    c.workspace_bytes = L.wrnn_taco_batch_workspace_bytes(S)
    return c


def test_header_and_binding_declare_the_batch_entry_points():
    _l, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    assert re.search(r'#define\s+WRNN_TACO_BATCH_MAX\s+8\b', hdr) and re.search(r'#define\s+WRNN_TACO_BATCH_NMAX\s+256\b', hdr)
    assert re.search(r'\}\s*wrnn_taco_batch_call\s*;', hdr)
    assert re.search(r'size_t\s+wrnn_taco_batch_workspace_bytes\s*\(\s*int32_t\s+n_sent\s*\)\s*;', hdr)
    assert re.search(r'int\s+wrnn_taco_decode_batch\s*\(\s*int\s+device\s*,\s*const\s+wrnn_taco_weights\s*\*\s*w\s*,\s*const\s+wrnn_taco_batch_call\s*\*\s*c\s*\)\s*;', hdr)
    assert re.search(r'#define\s+WRNN_ABI_VERSION\s+9\b', hdr) and L.wrnn_abi_version() == 9        # appended: the symbol tells
    for sym in ('wrnn_taco_batch_workspace_bytes', 'wrnn_taco_decode_batch'):
        assert sym in _l.EXPORTS and hasattr(L, sym), sym
    assert (_l.TACO_BATCH_MAX, _l.TACO_BATCH_NMAX) == (8, 256)
    # the struct as the header lays it out on an LP64 host: 5 x 4 bytes, pad, 6 pointers, steps_done, workspace, size, stream
    assert ctypes.sizeof(_l.TacoBatchCall) == 24 + 6 * 8 + 4 * 8
    assert _l.TacoBatchCall.n.offset == 24 and _l.TacoBatchCall.steps_done.offset == 72 and _l.TacoBatchCall.stream.offset == 96


def test_workspace_bytes_grow_with_the_sentences_and_refuse_a_count_out_of_range():
    _l, L = _lib()
    sizes = [L.wrnn_taco_batch_workspace_bytes(s) for s in range(1, 9)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:])), sizes
    assert len({b - a for a, b in zip(sizes, sizes[1:])}) == 1                 # one block of tagged vectors per sentence
    for bad in (0, -1, 9, 1000):
        assert L.wrnn_taco_batch_workspace_bytes(bad) == 0, bad


def _bad_n_sent(c, w, v):
    c.n_sent = v


def _bad_n(c, w, v):
    c.n[1] = v


def _bad_steps(c, w, v):
    c.max_steps[2] = v


def _bad_r(c, w, v):
    c.r, c.max_r = v


def _null_array(c, w, v):
    setattr(c, v, ctypes.cast(None, type(getattr(c, v))))


def _null_entry(c, w, v):
    getattr(c, v)[1] = None


def _null_field(c, w, v):
    setattr(c, v, None)


def _short_ws(c, w, v):
    c.workspace_bytes -= 1


def _geometry(c, w, v):
    setattr(w, v[0], v[1])


def _size(c, w, v):
    (c if v == 'call' else w).struct_bytes -= 8


@pytest.mark.parametrize('edit,value,needle', [
    (_size, 'call', 'struct size'), (_size, 'weights', 'struct size'),
    (_bad_n_sent, 0, '1..8'), (_bad_n_sent, 9, '1..8'), (_bad_n_sent, -3, '1..8'),
    (_bad_n, 0, 'sentence 1'), (_bad_n, 257, 'sentence 1'), (_bad_n, 1024, '256'),
    (_bad_steps, 0, 'sentence 2'), (_bad_steps, -5, 'sentence 2'),
    (_bad_r, (0, 20), 'r=0'), (_bad_r, (3, 2), 'max_r=2'), (_bad_r, (9, 20), '8'),
    (_null_array, 'n', 'null'), (_null_array, 'max_steps', 'null'), (_null_array, 'seq', 'null'), (_null_array, 'seq_proj', 'null'),
    (_null_array, 'mel_out', 'null'), (_null_array, 'scores_out', 'null'), (_null_field, 'steps_done', 'null'), (_null_field, 'workspace', 'null'),
    (_null_entry, 'seq', 'sentence 1'), (_null_entry, 'seq_proj', 'sentence 1'), (_null_entry, 'mel_out', 'sentence 1'),
    (_null_entry, 'scores_out', 'sentence 1'),
    (_short_ws, None, 'workspace'),
    (_geometry, ('lstm_dims', 256), 'geometry'), (_geometry, ('n_mels', 40), 'geometry'), (_geometry, ('attn_kernel', 15), 'geometry')],
    ids=lambda v: v.__name__.strip('_') if callable(v) else None)
def test_every_bad_argument_is_err_arg_with_a_message_before_any_device_call(edit, value, needle):
    """Device 10000 does not exist: a call that reached the HIP runtime would come back with another code than WRNN_ERR_ARG."""
    _l, L = _lib()
    w, c = _weights(_l), _call(_l, L)
    edit(c, w, value)
    assert L.wrnn_taco_decode_batch(10_000, ctypes.byref(w), ctypes.byref(c)) == _l.ERR_ARG
    msg = L.wrnn_taco_last_error().decode()
    assert needle in msg, msg


def test_null_arguments_and_the_first_check_past_validation():
    _l, L = _lib()
    w, c = _weights(_l), _call(_l, L)
    assert L.wrnn_taco_decode_batch(0, None, ctypes.byref(c)) == _l.ERR_ARG and b'null argument' in L.wrnn_taco_last_error()
    assert L.wrnn_taco_decode_batch(0, ctypes.byref(w), None) == _l.ERR_ARG and b'null argument' in L.wrnn_taco_last_error()
    # valid arguments, no such device: validation is passed and the DEVICE refuses -- any code but OK / WRNN_ERR_ARG, nothing was launched
    rc = L.wrnn_taco_decode_batch(10_000, ctypes.byref(w), ctypes.byref(c))
    assert rc not in (_l.WRNN_OK, _l.ERR_ARG), rc
    assert len(L.wrnn_taco_last_error()) > 0


def test_generate_batch_without_the_kernel_is_generate_per_sentence_bit_for_bit():
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    sig = inspect.signature(TacotronInference.generate_batch).parameters
    assert [sig[k].default for k in ('steps', 'kernel', 'cbhg_kernel', 'max_batch')] == [2000, True, False, 8]
    shapes = json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device='cpu')
    sents = [text_to_ids(t) for t in ('Hello there.', 'Hi.', 'One more, a little longer.')]
    outs = tts.generate_batch(sents, steps=5, kernel=False)
    assert len(outs) == 3
    for ids, (mel, lin, attn) in zip(sents, outs):
        m1, l1, a1 = tts.generate(ids, steps=5)
        assert mel.shape == (80, 5) and attn.shape == (5, len(ids))
        assert np.array_equal(mel, m1) and np.array_equal(lin, l1) and np.array_equal(attn, a1)
    # the kernel form has no host fallback; max_batch is checked where it is used
    with pytest.raises(_lib.WrnnError):
        tts.generate_batch(sents, steps=5)
    with pytest.raises(ValueError):
        tts.generate_batch(sents, steps=5, max_batch=9)
    # the decoder's weight struct is built once per instance
    if os.path.exists(_lib.SO_PATH):
        assert tts.decoder_weights() is tts.decoder_weights()
        assert tts.decoder_weights().lstm_dims == 512 and tts.decoder_weights().encoder_width == 256
