"""The encoder / post-net entry points of the C ABI (csrc/wrnn_cbhg.hip: wrnn_taco_front_*, wrnn_taco_encode, wrnn_taco_postnet) and their
Python switch (`TacotronInference.generate(..., cbhg_kernel=...)`) without a GPU: they fail loudly, with a code and a message, never crash
and never compute on the host."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from helpers import GOLDEN


def _lib():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def _shipped_weights(_lib, ptr=0x1000):
    """A wrnn_taco_front_weights with the reference's dims and `ptr` in every pointer create checks (never dereferenced before the
    device check)."""
    w = _lib.TacoFrontWeights()
    w.struct_bytes = ctypes.sizeof(_lib.TacoFrontWeights)
    w.n_symbols, w.embed_dims, w.prenet1, w.prenet2, w.encoder_proj_dims, w.n_mels, w.fft_bins = 148, 256, 256, 128, 256, 80, 80
    for n in ('embedding', 'prenet_fc1_w', 'prenet_fc1_b', 'prenet_fc2_w', 'prenet_fc2_b', 'encoder_proj_w', 'post_proj_w'):
        setattr(w, n, ptr)
    for c, (K, cin, p1) in ((w.encoder_cbhg, (16, 128, 128)), (w.postnet, (8, 80, 256))):
        c.K, c.in_channels, c.proj1_channels, c.proj2_channels, c.channels, c.num_highways = K, cin, p1, cin, 128, 4
        for name, ctype in _lib.CbhgWeights._fields_:
            if ctype is ctypes.c_void_p:
                setattr(c, name, ptr)
            elif ctype is not ctypes.c_int32:
                for i in range(K if name.startswith('bank') else 4):
                    getattr(c, name)[i] = ptr
    w.encoder_cbhg.pre_highway_w = None                 # 128 == channels: no pre_highway in the encoder
    return w


def test_front_entry_points_fail_loudly_without_a_front():
    _l, L = _lib()
    for sym in ('wrnn_taco_front_create', 'wrnn_taco_front_destroy', 'wrnn_taco_front_workspace_bytes', 'wrnn_taco_encode', 'wrnn_taco_postnet'):
        assert hasattr(L, sym), sym
        assert sym in _l.EXPORTS
    assert L.wrnn_abi_version() == 9
    h = ctypes.c_void_p()
    assert L.wrnn_taco_front_create(None, 0, ctypes.byref(h)) == _l.ERR_ARG
    assert b'NULL' in L.wrnn_taco_last_error()
    assert L.wrnn_taco_front_create(ctypes.byref(_shipped_weights(_l)), 0, None) == _l.ERR_ARG
    L.wrnn_taco_front_destroy(None)
    assert L.wrnn_taco_front_workspace_bytes(None, 100) == 0
    assert L.wrnn_taco_encode(None, None, 10, None, None, None, None, 0, None) == _l.ERR_ARG
    assert L.wrnn_taco_postnet(None, None, 10, None, None, None, 0, None) == _l.ERR_ARG
    assert b'NULL' in L.wrnn_taco_last_error()


@pytest.mark.parametrize('field,value,where', [
    ('struct_bytes', 8, None), ('embed_dims', 200, None), ('fft_bins', 0, None), ('prenet2', 64, None), ('n_symbols', 0, None),
    ('K', 17, 'encoder_cbhg'), ('K', 0, 'postnet'), ('in_channels', 120, 'encoder_cbhg'), ('proj1_channels', 250, 'postnet'),
    ('proj2_channels', 96, 'postnet'), ('channels', 256, 'encoder_cbhg'), ('num_highways', 5, 'postnet'), ('pre_highway_w', None, 'postnet'),
    ('pre_highway_w', 0x1000, 'encoder_cbhg'), ('rnn_w_hh_rev', None, 'encoder_cbhg'), ('embedding', None, None)])
def test_front_create_refuses_bad_dims_with_a_message(field, value, where):
    """Unsupported dims and NULL pointers are WRNN_ERR_ARG with a text, before any device is touched (so also without one)."""
    _l, L = _lib()
    w = _shipped_weights(_l)
    setattr(getattr(w, where) if where else w, field, value)
    h = ctypes.c_void_p()
    assert L.wrnn_taco_front_create(ctypes.byref(w), 0, ctypes.byref(h)) == _l.ERR_ARG
    assert len(L.wrnn_taco_last_error()) > 0 and not h.value


def test_front_create_without_the_device_is_no_device():
    """Valid dims, but no such device: WRNN_ERR_NO_DEVICE before any weight pointer is read (device 0 too on a host without a GPU)."""
    _l, L = _lib()
    for device in [10_000, -1] + ([] if torch.cuda.is_available() else [0]):
        h = ctypes.c_void_p()
        assert L.wrnn_taco_front_create(ctypes.byref(_shipped_weights(_l)), device, ctypes.byref(h)) == _l.ERR_NO_DEVICE
        assert b'no HIP device' in L.wrnn_taco_last_error() and not h.value


def test_generate_keeps_the_torch_ops_by_default_and_refuses_the_kernels_on_the_cpu():
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    assert inspect.signature(TacotronInference.generate).parameters['cbhg_kernel'].default is False
    shapes = json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device='cpu')
    ids = text_to_ids('Hi.')
    tts.generate(ids, steps=2)
    assert tts.last_front_path == 'torch'
    with pytest.raises(_lib.WrnnError):
        tts.generate(ids, steps=2, cbhg_kernel=True)
    with pytest.raises(_lib.WrnnError):
        tts.encode_kernel(ids)
