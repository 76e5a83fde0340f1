"""CPU tests of `wrnn_pre_upsample_many`'s argument checks (include/wavernn_amd.h): a bad table or a short workspace is WRNN_ERR_ARG before anything
is launched.  The handle is the dims-only one of `wrnn_pre_debug_host_handle` (no device is looked for), on which a call that PASSES its argument
checks answers WRNN_ERR_NO_DEVICE -- so an ERR_ARG here was raised in front of every launch."""
import ctypes

import pytest

from wavernn_amd import _lib

ERR_ARG, ERR_NO_DEVICE = -1, -2
FAKE = 0x10000            # a non-NULL, 256-byte aligned "device pointer": the checks never read through it


@pytest.fixture(scope='module')
def L():
    return _lib.lib()


@pytest.fixture(scope='module')
def handle(L):
    pw = _lib.PreWeights()
    pw.feat_dims, pw.compute_dims, pw.res_out_dims, pw.res_blocks, pw.pad = 80, 128, 128, 10, 2
    for i, s in enumerate((5, 5, 11)):
        pw.upsample_factors[i] = s
    pre = ctypes.c_void_p()
    assert L.wrnn_pre_debug_host_handle(ctypes.byref(pw), ctypes.byref(pre)) == 0
    yield pre
    L.wrnn_pre_destroy(pre)


def _table(frames):
    tab = (_lib.PreUtt * len(frames))()
    up = aux = 0
    for k, n in enumerate(frames):
        tab[k].mel, tab[k].n_frames, tab[k].up_row, tab[k].aux_row = FAKE, n, up, aux
        up, aux = up + max(n, 0) * 275, aux + max(n, 0)
    return tab


def _call(L, handle, tab, n, ws_bytes, rows=0):
    return L.wrnn_pre_upsample_many(handle, tab, n, rows, FAKE, FAKE, FAKE, ws_bytes, None)


def test_host_handle_answers_the_size_queries(L, handle):
    assert L.wrnn_pre_hop(handle) == 275
    tab = _table([1, 16, 17, 53])
    one = [L.wrnn_pre_workspace_bytes(handle, n) for n in (1, 16, 17, 53)]
    full, rows = L.wrnn_pre_workspace_bytes_many(handle, tab, 4, 0), L.wrnn_pre_workspace_bytes_many(handle, tab, 4, 1)
    # table (5 entries of 64 B -> 512 B) + per utterance stage 1 [+ stage 2], each rounded up to 256 B
    al = lambda x: (x + 255) // 256 * 256
    s1 = [al((n + 4) * 5 * 80 * 4) for n in (1, 16, 17, 53)]
    s2 = [al((n + 4) * 25 * 80 * 4) for n in (1, 16, 17, 53)]
    assert rows == 512 + sum(s1) and full == rows + sum(s2)
    assert full <= 512 + sum(al(b) for b in one)                   # never more than the per-utterance workspaces side by side
    assert L.wrnn_pre_workspace_bytes_many(None, tab, 4, 0) == 0 and L.wrnn_pre_workspace_bytes_many(handle, None, 4, 0) == 0
    assert L.wrnn_pre_workspace_bytes_many(handle, tab, 0, 0) == 0
    assert L.wrnn_pre_workspace_bytes_many(handle, _table([16, 0]), 2, 0) == 0


def test_good_arguments_reach_the_device_check(L, handle):
    """The control of the tests below: the same call with nothing wrong gets past the argument checks (and finds no device on this handle)."""
    tab = _table([1, 16, 17, 53])
    for rows in (0, 1):
        need = L.wrnn_pre_workspace_bytes_many(handle, tab, 4, rows)
        assert _call(L, handle, tab, 4, need, rows) == ERR_NO_DEVICE, L.wrnn_pre_last_error()
    assert L.wrnn_pre_upsample(handle, FAKE, 16, FAKE, FAKE, FAKE, L.wrnn_pre_workspace_bytes(handle, 16), None) == ERR_NO_DEVICE


def test_null_table(L, handle):
    assert _call(L, handle, None, 4, 1 << 30) == ERR_ARG
    assert b'table' in L.wrnn_pre_last_error()
    assert L.wrnn_pre_upsample_many(None, _table([16]), 1, 0, FAKE, FAKE, FAKE, 1 << 30, None) == ERR_ARG


def test_zero_utterances(L, handle):
    tab = _table([16])
    for n in (0, -1):
        assert _call(L, handle, tab, n, 1 << 30) == ERR_ARG
        assert b'utterance count' in L.wrnn_pre_last_error()


@pytest.mark.parametrize('bad', [0, -5])
def test_n_frames_below_one(L, handle, bad):
    tab = _table([16, bad, 17])
    assert _call(L, handle, tab, 3, 1 << 30) == ERR_ARG
    assert b'utterance 1: bad n_frames' in L.wrnn_pre_last_error()


@pytest.mark.parametrize('rows', [0, 1])
def test_workspace_too_small(L, handle, rows):
    tab = _table([1, 16, 17, 53])
    need = L.wrnn_pre_workspace_bytes_many(handle, tab, 4, rows)
    assert need > 0
    assert _call(L, handle, tab, 4, need - 1, rows) == ERR_ARG
    assert b'workspace too small' in L.wrnn_pre_last_error()
    assert _call(L, handle, tab, 4, 0, rows) == ERR_ARG
