"""CPU tests of the many-sentence encoder / post-net entry points (include/wavernn_amd.h: wrnn_taco_front_workspace_bytes_many,
wrnn_taco_encode_many, wrnn_taco_postnet_many, wrnn_bigru_many) on the dims-only handle of `wrnn_taco_front_debug_host_handle`: the size
query, and the argument checks, which answer WRNN_ERR_ARG / WRNN_ERR_WORKSPACE before anything is launched.  A call that PASSES its checks
answers WRNN_ERR_NO_DEVICE on that handle -- so every other code here was raised in front of every launch."""
import ctypes
import json
import os

import pytest

from helpers import GOLDEN
from wavernn_amd import _lib

ERR_ARG, ERR_NO_DEVICE, ERR_WORKSPACE = -1, -2, -4
FAKE = 0x10000            # a non-NULL, 256-byte aligned "device pointer": the checks never read through it
NEW = ('wrnn_taco_front_workspace_bytes_many', 'wrnn_taco_encode_many', 'wrnn_taco_postnet_many', 'wrnn_bigru_many',
       'wrnn_taco_front_debug_host_handle')


@pytest.fixture(scope='module')
def L():
    return _lib.lib()


def _shipped_dims():
    """A wrnn_taco_front_weights with the reference's dims and every pointer NULL (the dims-only handle reads none)."""
    w = _lib.TacoFrontWeights()
    w.struct_bytes = ctypes.sizeof(_lib.TacoFrontWeights)
    w.n_symbols, w.embed_dims, w.prenet1, w.prenet2, w.encoder_proj_dims, w.n_mels, w.fft_bins = 148, 256, 256, 128, 256, 80, 80
    for c, (K, cin, p1) in ((w.encoder_cbhg, (16, 128, 128)), (w.postnet, (8, 80, 256))):
        c.K, c.in_channels, c.proj1_channels, c.proj2_channels, c.channels, c.num_highways = K, cin, p1, cin, 128, 4
    return w


@pytest.fixture(scope='module')
def handle(L):
    h = ctypes.c_void_p()
    assert L.wrnn_taco_front_debug_host_handle(ctypes.byref(_shipped_dims()), ctypes.byref(h)) == 0, L.wrnn_taco_last_error()
    assert h.value
    yield h
    L.wrnn_taco_front_destroy(h)


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def _bytes_many(L, handle, lengths, n_sent=None):
    return L.wrnn_taco_front_workspace_bytes_many(handle, _i32(lengths), len(lengths) if n_sent is None else n_sent)


def _encode(L, handle, lengths, n_sent=None, ws=FAKE, ws_bytes=None, seq=FAKE, proj=FAKE, pre=None, table=True):
    n = _i32(lengths) if table else None
    k = len(lengths) if n_sent is None else n_sent
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return L.wrnn_taco_encode_many(handle, FAKE, n, k, seq, proj, pre, ws, ws_bytes, None)


def _postnet(L, handle, lengths, n_sent=None, mels=None, ws=FAKE, ws_bytes=None, linear=FAKE, pre=None):
    k = len(lengths) if n_sent is None else n_sent
    ptrs = (ctypes.c_void_p * len(lengths))(*([FAKE] * len(lengths) if mels is None else mels))
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return L.wrnn_taco_postnet_many(handle, ptrs, _i32(lengths), k, linear, pre, ws, ws_bytes, None)


def test_new_symbols_are_exported_and_the_abi_version_stays(L):
    for sym in NEW:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTS, sym
    assert L.wrnn_abi_version() == 9 == _lib.ABI_VERSION
    assert _lib.TACO_FRONT_MANY_MAX == 64


def test_host_handle_refuses_bad_dims_and_reads_no_pointer(L):
    w = _shipped_dims()
    w.embed_dims = 200
    h = ctypes.c_void_p()
    assert L.wrnn_taco_front_debug_host_handle(ctypes.byref(w), ctypes.byref(h)) == ERR_ARG and not h.value
    assert len(L.wrnn_taco_last_error()) > 0
    assert L.wrnn_taco_front_debug_host_handle(None, ctypes.byref(h)) == ERR_ARG
    assert L.wrnn_taco_front_debug_host_handle(ctypes.byref(_shipped_dims()), None) == ERR_ARG


def test_workspace_bytes_many_is_zero_for_a_bad_table(L, handle):
    assert L.wrnn_taco_front_workspace_bytes_many(handle, None, 3) == 0
    assert L.wrnn_taco_front_workspace_bytes_many(None, _i32([5]), 1) == 0
    assert _bytes_many(L, handle, [5], 0) == 0
    assert _bytes_many(L, handle, [5] * 65) == 0
    assert _bytes_many(L, handle, [5] * 64) > 0
    assert _bytes_many(L, handle, [16, 0, 17]) == 0
    assert _bytes_many(L, handle, [16, -3]) == 0
    assert _bytes_many(L, handle, [(1 << 20) + 1]) == 0
    assert _bytes_many(L, handle, [1 << 20]) > 0


@pytest.mark.parametrize('n', [1, 15, 16, 17, 100, 800])
def test_workspace_bytes_many_of_one_sentence_covers_the_single_call(L, handle, n):
    one = L.wrnn_taco_front_workspace_bytes(handle, n)
    assert one > 0 and _bytes_many(L, handle, [n]) >= one


def test_workspace_bytes_many_grows_with_every_length_in_steps_of_256(L, handle):
    base = [17, 1, 16, 33]
    b0 = _bytes_many(L, handle, base)
    assert b0 > 0 and b0 % 256 == 0
    for k in range(len(base)):
        prev = b0
        for add in (1, 2, 15, 16, 100):
            grown = list(base)
            grown[k] += add
            b = _bytes_many(L, handle, grown)
            assert b % 256 == 0 and b >= prev, (k, add, b, prev)
            prev = b
    assert _bytes_many(L, handle, base + [1]) >= b0


def test_valid_calls_reach_the_device_check(L, handle):
    """The control of the tests below: nothing wrong -> past the argument checks, and no device on this handle."""
    lengths = [17, 1, 16, 33]
    need = _bytes_many(L, handle, lengths)
    assert _encode(L, handle, lengths, ws_bytes=need) == ERR_NO_DEVICE, L.wrnn_taco_last_error()
    assert b'dims-only' in L.wrnn_taco_last_error()
    assert _encode(L, handle, lengths, ws_bytes=need, pre=FAKE) == ERR_NO_DEVICE
    assert _postnet(L, handle, lengths, ws_bytes=need) == ERR_NO_DEVICE, L.wrnn_taco_last_error()
    assert _postnet(L, handle, lengths, ws_bytes=need, pre=FAKE) == ERR_NO_DEVICE
    assert _encode(L, handle, [5] * 64) == ERR_NO_DEVICE and _postnet(L, handle, [5] * 64) == ERR_NO_DEVICE
    # the single-sentence entry points answer the same way on this handle
    one = L.wrnn_taco_front_workspace_bytes(handle, 17)
    assert L.wrnn_taco_encode(handle, FAKE, 17, FAKE, FAKE, None, FAKE, one, None) == ERR_NO_DEVICE
    assert L.wrnn_taco_postnet(handle, FAKE, 17, FAKE, None, FAKE, one, None) == ERR_NO_DEVICE


@pytest.mark.parametrize('call', [_encode, _postnet])
def test_sentence_count_outside_1_to_64(L, handle, call):
    assert call(L, handle, [5], n_sent=0) == ERR_ARG
    assert b'sentence count 0' in L.wrnn_taco_last_error() and b'64' in L.wrnn_taco_last_error()
    assert call(L, handle, [5] * 65) == ERR_ARG
    assert b'sentence count 65' in L.wrnn_taco_last_error()
    assert call(L, handle, [5], n_sent=-1) == ERR_ARG


@pytest.mark.parametrize('call', [_encode, _postnet])
@pytest.mark.parametrize('bad', [0, -4, (1 << 20) + 1])
def test_length_outside_its_range_names_the_sentence(L, handle, call, bad):
    assert call(L, handle, [16, 17, bad, 5]) == ERR_ARG
    msg = L.wrnn_taco_last_error()
    assert b'sentence 2' in msg and str(bad).encode() in msg and str(1 << 20).encode() in msg, msg


def test_null_handle_table_or_output(L, handle):
    assert _encode(L, None, [5]) == ERR_ARG and len(L.wrnn_taco_last_error()) > 0
    assert _encode(L, handle, [5], table=False) == ERR_ARG and b'table' in L.wrnn_taco_last_error()
    assert _encode(L, handle, [5], seq=None) == ERR_ARG and _encode(L, handle, [5], proj=None) == ERR_ARG
    assert _encode(L, handle, [5], ws=None) == ERR_ARG
    assert L.wrnn_taco_encode_many(handle, None, _i32([5]), 1, FAKE, FAKE, None, FAKE, 1 << 40, None) == ERR_ARG
    assert _postnet(L, None, [5]) == ERR_ARG
    assert _postnet(L, handle, [5], linear=None) == ERR_ARG and _postnet(L, handle, [5], ws=None) == ERR_ARG
    assert L.wrnn_taco_postnet_many(handle, None, _i32([5]), 1, FAKE, None, FAKE, 1 << 40, None) == ERR_ARG
    assert b'mel' in L.wrnn_taco_last_error()
    assert L.wrnn_taco_postnet_many(handle, (ctypes.c_void_p * 1)(FAKE), None, 1, FAKE, None, FAKE, 1 << 40, None) == ERR_ARG
    assert len(L.wrnn_taco_last_error()) > 0


def test_null_mel_of_one_sentence(L, handle):
    assert _postnet(L, handle, [16, 17, 5], mels=[FAKE, None, FAKE]) == ERR_ARG
    msg = L.wrnn_taco_last_error()
    assert b'sentence 1' in msg and b'mel' in msg, msg


def test_misaligned_output_or_workspace(L, handle):
    for kw in (dict(seq=FAKE + 1), dict(proj=FAKE + 1), dict(pre=FAKE + 1), dict(seq=FAKE + 8)):
        assert _encode(L, handle, [16, 5], **kw) == ERR_ARG, kw
        assert b'16-byte' in L.wrnn_taco_last_error()
    for kw in (dict(linear=FAKE + 1), dict(pre=FAKE + 1)):
        assert _postnet(L, handle, [16, 5], **kw) == ERR_ARG, kw
        assert b'16-byte' in L.wrnn_taco_last_error()
    for call in (_encode, _postnet):
        assert call(L, handle, [16, 5], ws=FAKE + 128) == ERR_ARG
        assert b'256-byte' in L.wrnn_taco_last_error()
        assert call(L, handle, [16, 5], ws=FAKE + 16) == ERR_ARG


@pytest.mark.parametrize('call', [_encode, _postnet])
def test_workspace_one_byte_short(L, handle, call):
    lengths = [17, 1, 16, 33]
    need = _bytes_many(L, handle, lengths)
    assert call(L, handle, lengths, ws_bytes=need - 1) == ERR_WORKSPACE
    assert b'workspace too small' in L.wrnn_taco_last_error()
    assert call(L, handle, lengths, ws_bytes=0) == ERR_WORKSPACE
    assert call(L, handle, lengths, ws_bytes=need) == ERR_NO_DEVICE


def _bigru_many(T, n_seq=None, **over):
    c = _lib.BigruManyCall()
    c.struct_bytes = ctypes.sizeof(_lib.BigruManyCall)
    c.n_seq, c.hidden = len(T) if n_seq is None else n_seq, 128
    c.T = _i32(T)
    for name in ('gi_fwd', 'gi_rev', 'w_hh_fwd', 'w_hh_rev', 'b_hh_fwd', 'b_hh_rev', 'out'):
        setattr(c, name, FAKE)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_bigru_many_argument_checks(L):
    rc = lambda c: L.wrnn_bigru_many(0, ctypes.byref(c))
    assert L.wrnn_bigru_many(0, None) == ERR_ARG
    assert rc(_bigru_many([1, 2, 19], struct_bytes=8)) == ERR_ARG and b'struct size' in L.wrnn_taco_last_error()
    assert rc(_bigru_many([5], n_seq=0)) == ERR_ARG and b'n_seq=0' in L.wrnn_taco_last_error()
    assert rc(_bigru_many([5] * 65)) == ERR_ARG and b'n_seq=65' in L.wrnn_taco_last_error()
    assert rc(_bigru_many([1, 0, 19])) == ERR_ARG and b'sequence 1' in L.wrnn_taco_last_error()
    assert rc(_bigru_many([1, (1 << 20) + 1])) == ERR_ARG
    assert rc(_bigru_many([1, 2], hidden=256)) == ERR_ARG
    for name in ('gi_fwd', 'gi_rev', 'w_hh_fwd', 'w_hh_rev', 'b_hh_fwd', 'b_hh_rev', 'out'):
        assert rc(_bigru_many([1, 2, 19], **{name: None})) == ERR_ARG, name
        assert len(L.wrnn_taco_last_error()) > 0
    c = _bigru_many([1, 2])
    c.T = None
    assert rc(c) == ERR_ARG


def test_generate_batch_refuses_the_kernels_on_the_cpu():
    """`generate_batch(cbhg_kernel=True)` on a CPU model raises, as `generate` does; so do the `_many` methods."""
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    shapes = json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device='cpu')
    ids = text_to_ids('Hi.')
    with pytest.raises(_lib.WrnnError):
        tts.generate_batch([ids, ids], steps=2, cbhg_kernel=True)
    with pytest.raises(_lib.WrnnError):
        tts.encode_kernel_many([ids, ids])
    with pytest.raises(_lib.WrnnError):
        import torch
        tts.postnet_kernel_many([torch.zeros(80, 3)])
