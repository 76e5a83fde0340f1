"""`wrnn_post_chunk_host` -- the post-loop stage of a step range, by the calling thread -- against the numpy helpers of fold.py (which
test_host_logic.py pins to the reference's waveforms), bit for bit, and the argument checks of both forms.  CPU-only; tests/test_gpu_unbatched.py
runs the device form on the same inputs."""
import ctypes
import os
import re

import numpy as np
import pytest

import unbatched_cases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_or_build():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    _lib, L = _lib_or_build()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read(), flags=re.S)
    for sym in ('wrnn_post_chunk', 'wrnn_post_chunk_host'):
        assert sym in _lib.EXPORTS and hasattr(L, sym) and re.search(r'\bint\s+%s\s*\(\s*const\s+wrnn_post_chunk_call\s*\*\s*c\s*\)\s*;' % sym, hdr), sym
    assert re.search(r'\}\s*wrnn_post_chunk_call\s*;', hdr)
    assert L.wrnn_abi_version() == 9 == _lib.ABI_VERSION and re.search(r'#define\s+WRNN_ABI_VERSION\s+9\b', hdr)       # appended: the symbol tells
    # the struct as the header lays it out on an LP64 host: 7 x 4 bytes, pad, 8 pointers
    assert ctypes.sizeof(_lib.PostChunkCall) == 32 + 8 * 8 and _lib.PostChunkCall.segments.offset == 32 and _lib.PostChunkCall.stream.offset == 88


def _call(**kw):
    _lib, _ = _lib_or_build()
    n, T, w = 2, 12, 5
    bufs = dict(segments=np.zeros((n, T), np.float32), wave_len=np.array([8, 12], np.int32), tail=np.linspace(1, 0, 4), lut=np.linspace(-1, 1, 4),
                out64=np.full((n, w), 123.0), out32=np.full((n, w), 123.0, np.float32), row=np.array([1, 0], np.int32))
    c = _lib.PostChunkCall(n_utt=n, T=T, t0=3, t1=3 + w, n_classes=4, tail_len=4, **{k: v.ctypes.data for k, v in bufs.items()})
    for k, v in kw.items():
        if k == 'wave_len_values':
            bufs['wave_len'][:] = v
        else:
            setattr(c, k, v)
    return c, bufs


BAD_CALLS = [
    (dict(struct_bytes=8), 'struct_bytes is 8'),
    (dict(segments=None), 'NULL segments'),
    (dict(wave_len=None), 'NULL wave_len'),
    (dict(tail=None), 'NULL tail'),
    (dict(out64=None, out32=None), 'out64 and out32 are both NULL'),
    (dict(n_utt=0), 'n_utt < 1'),
    (dict(t0=-1), 'bad step range'),
    (dict(t0=8), 'bad step range'),                    # t0 == t1
    (dict(t0=9), 'bad step range'),
    (dict(t1=13), 'bad step range'),                   # t1 > T
    (dict(tail_len=-1), 'tail_len < 0'),
    (dict(n_classes=1), 'lut with n_classes < 2'),
]


@pytest.mark.parametrize('entry', ['wrnn_post_chunk', 'wrnn_post_chunk_host'])
@pytest.mark.parametrize('fields,message', BAD_CALLS, ids=[f'{m}-{i}' for i, (_, m) in enumerate(BAD_CALLS)])
def test_bad_arguments_are_refused_before_anything_runs(entry, fields, message):
    _lib, L = _lib_or_build()
    c, bufs = _call(**fields)
    assert getattr(L, entry)(ctypes.byref(c)) == _lib.ERR_ARG
    assert message in L.wrnn_post_last_error().decode(), L.wrnn_post_last_error()
    assert (bufs['out64'] == 123.0).all() and (bufs['out32'] == 123.0).all()
    assert getattr(L, entry)(None) == _lib.ERR_ARG and b'NULL' in L.wrnn_post_last_error()


def test_host_form_refuses_what_only_it_can_read_and_takes_the_rest():
    _lib, L = _lib_or_build()
    c, bufs = _call(wave_len_values=[8, 3])            # wave_len < tail_len: the reference's tail fade raises there
    assert L.wrnn_post_chunk_host(ctypes.byref(c)) == _lib.ERR_ARG and b'wave_len 3 < tail_len 4' in L.wrnn_post_last_error()
    assert (bufs['out64'] == 123.0).all()
    with pytest.raises(_lib.WrnnError, match='wave_len 3 < tail_len 4'):
        _lib.post_chunk_host(bufs['segments'], [8, 3], 3, 8, bufs['tail'])
    # valid: lut without n_classes is the only use of n_classes; one output suffices; tail_len 0 fades nothing
    for kw in (dict(lut=None, n_classes=0), dict(out64=None), dict(out32=None), dict(row=None), dict(tail_len=0)):
        c, bufs = _call(**kw)
        assert L.wrnn_post_chunk_host(ctypes.byref(c)) == _lib.WRNN_OK, kw
        assert ('out64' in kw) == (bufs['out64'] == 123.0).all() and ('out32' in kw) == (bufs['out32'] == 123.0).all()


_REF = {}


def _case(kind, row):
    """the inputs and the reference waveform of a case, computed once"""
    from wavernn_amd.post import chunk_host_tables
    key = (kind, None if row is None else tuple(row))
    if key not in _REF:
        seg, mu_law = U.segments(kind)
        tail, lut = chunk_host_tables(U.HOP, U.C, mu_law)
        ref = U.reference(seg, mu_law, row)
        ref.setflags(write=False)
        _REF[key] = (seg, tail, lut, ref)
    return _REF[key]


@pytest.mark.parametrize('row', U.ROWS, ids=['row-null', 'row-permuted'])
@pytest.mark.parametrize('ranges', sorted(U.RANGES))
@pytest.mark.parametrize('kind', ['mol', 'raw_lut', 'raw'])
def test_host_form_is_the_reference_waveform_bit_for_bit(kind, ranges, row):
    _lib, _ = _lib_or_build()
    seg, tail, lut, ref = _case(kind, row)
    assert len(tail) == U.TAIL_LEN and (lut is None) == (kind != 'raw_lut')
    got = []
    for t0, t1 in U.RANGES[ranges]:
        o64, o32 = _lib.post_chunk_host(seg, U.WAVE_LEN, t0, t1, tail, lut, row=row, want32=True)
        assert o64.shape == o32.shape == (3, t1 - t0) and o64.dtype == np.float64 and o32.dtype == np.float32
        assert np.array_equal(o64, ref[:, t0:t1]), (t0, t1, np.abs(o64 - ref[:, t0:t1]).max())
        assert np.array_equal(o32, o64.astype(np.float32))
        for u in range(3):
            assert not o64[u, max(0, int(U.WAVE_LEN[u]) - t0):].any() and not o32[u, max(0, int(U.WAVE_LEN[u]) - t0):].any()
        got.append(o64)
    if U.RANGES[ranges][0][0] == 0 and U.RANGES[ranges][-1][1] == U.T and ranges != 'fade-from-step-0':
        assert np.array_equal(np.concatenate(got, axis=1), ref)            # the chunks, concatenated, are the waveforms
    if ranges == 'past-a-short-one':
        assert not got[0][0].any() and not got[1].any()
    if ranges == 'fade-from-step-0':                                        # row 0 is faded from its first sample on
        r0 = 0 if row is None else int(row[0])
        val = (lambda y: float(lut[int(round((float(y) + 1) * (U.C - 1) / 2))]) if lut is not None else float(y))
        assert got[0][0, 0] == val(seg[r0, 0]) * tail[0] and tail[0] == 1.0 and got[0][0, 1] == val(seg[r0, 1]) * tail[1] and tail[1] < 1.0
