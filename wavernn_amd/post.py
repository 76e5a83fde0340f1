"""Post-loop stage on the device (`wrnn_post_unfold`, include/wavernn_amd.h): float64 gather cast, mu-law expansion,
cross-fade + overlap-add and tail fade of `WaveRNN.generate()` (reference models/fatchord_version.py:245-258, :342-405,
utils/dsp.py:98-103) for any number of utterances in one launch.

Bit-exact with the reference by construction: the transcendental parts (pow of `decode_mu_law`, sqrt / linspace of the
fades) are evaluated here with the reference's numpy expressions and uploaded as float64 tables; the kernel only gathers,
multiplies and adds doubles in the reference's order."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import fold as _fold

_tables = {}


def _fade_tables(overlap, hop, device):
    key = ('fade', overlap, hop, str(device))
    if key not in _tables:
        silence_len = overlap // 2
        fade_len = overlap - silence_len
        t = np.linspace(-1, 1, fade_len, dtype=np.float64)                       # reference :381-392
        fade_in = np.concatenate([np.zeros(silence_len, np.float64), np.sqrt(0.5 * (1 + t))])
        fade_out = np.concatenate([np.ones(silence_len, np.float64), np.sqrt(0.5 * (1 - t))])
        tail = np.linspace(1, 0, 20 * hop)                                       # reference :256
        _tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (fade_in, fade_out, tail))
    return _tables[key]


def _mu_law_lut(n_classes, device):
    key = ('lut', n_classes, str(device))
    if key not in _tables:
        idx = np.arange(n_classes, dtype=np.float32)
        y32 = np.float32(2.0) * idx / np.float32(n_classes - 1) - np.float32(1.0)    # the loop's float32 sample (:237)
        lut = _fold.decode_mu_law(y32.astype(np.float64), n_classes, False)           # utils/dsp.py:98-103, float64
        _tables[key] = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float64)).to(device)
    return _tables[key]


class UnfoldTables:
    """Everything `wrnn_post_unfold` reads besides the segments, on the device: it depends on the plan only (which utterance owns which segments, the
    wave lengths, overlap / hop / classes), so `prepare_unfold` can put it there BEFORE the loop is queued -- one copy from a page-locked staging array
    (offsets int64, then first / folds int32), the cached fade and mu-law tables, the output buffer.  Nothing then lies between the last loop launch and
    the unfold launch but the launch itself."""

    def __init__(self, first, folds, wave_lens, overlap, hop, n_classes, mu_law, batched, dev):
        self.tail_len = 20 * hop
        if min(wave_lens) < self.tail_len:
            raise ValueError(f'operands could not be broadcast together with shapes ({min(wave_lens)},) ({self.tail_len},)')
        n = self.n_utt = len(wave_lens)
        self.off = np.concatenate([[0], np.cumsum(wave_lens)]).astype(np.int64)
        stage = torch.empty(8 * (n + 1) + 8 * n, dtype=torch.uint8, pin_memory=True)
        h = stage.numpy()
        h[:8 * (n + 1)] = self.off.view(np.uint8)
        h[8 * (n + 1):] = np.concatenate([np.asarray(first, np.int32), np.asarray(folds, np.int32)]).view(np.uint8)
        self.tabs = stage.to(dev, non_blocking=True)         # (the caching host allocator keeps the pages until the copy has run)
        self.overlap, self.batched, self.n_classes = (overlap if batched else 0), bool(batched), n_classes
        self.fade_in, self.fade_out, self.tail = _fade_tables(self.overlap, hop, dev)
        self.lut = _mu_law_lut(n_classes, dev) if mu_law else None
        self.out = torch.empty(int(self.off[-1]), dtype=torch.float64, device=dev)
        self.key = (tuple(int(x) for x in first), tuple(int(x) for x in folds), tuple(int(x) for x in wave_lens))


def prepare_unfold(first, folds, wave_lens, overlap, hop, n_classes, mu_law, batched=True, device='cuda'):
    """The tables of `unfold_on_device(..., tables=...)` for these utterances, uploaded now, on the current stream."""
    return UnfoldTables(first, folds, wave_lens, overlap, hop, n_classes, mu_law, batched, torch.device(device))


def unfold_on_device(segments, first, folds, wave_lens, overlap, hop, n_classes, mu_law, batched=True, tables=None):
    """segments: float32 CUDA (n, T).  Utterance u owns rows [first[u], first[u]+folds[u]).  Returns a float64 CUDA tensor
    of all waveforms concatenated and the list of (start, end) slices.  Raises ValueError where the reference's tail
    fade would (wave_len < 20*hop, :258).  tables: what `prepare_unfold` made for the same utterances earlier (None: made here)."""
    dev = segments.device
    t = tables
    if t is None:
        t = UnfoldTables(first, folds, wave_lens, overlap, hop, n_classes, mu_law, batched, dev)
    elif t.key != (tuple(int(x) for x in first), tuple(int(x) for x in folds), tuple(int(x) for x in wave_lens)) or t.lut is None and mu_law:
        raise ValueError('unfold tables prepared for other utterances')
    L = _lib.lib()
    n_utt, T, off = t.n_utt, int(segments.shape[1]), t.off
    segments = segments.contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p_off = t.tabs.data_ptr()
    p_first = p_off + 8 * (n_utt + 1)
    rc = L.wrnn_post_unfold(segments.data_ptr(), T, n_utt, p_first, p_first + 4 * n_utt, p_off,
                            t.lut.data_ptr() if t.lut is not None else None, n_classes, t.fade_in.data_ptr(), t.fade_out.data_ptr(),
                            t.overlap, t.tail.data_ptr(), t.tail_len, 1 if t.batched else 0, t.out.data_ptr(), stream)
    if rc != 0:
        raise _lib.WrnnError(f'wrnn_post_unfold failed (rc={rc}): {L.wrnn_post_last_error().decode()}')
    return t.out, [(int(off[u]), int(off[u + 1])) for u in range(n_utt)]


def chunk_host_tables(hop, n_classes, mu_law):
    """(tail, lut or None): the float64 host tables of `_lib.post_chunk_host` -- the reference's numpy expressions, what the device tables are copies of."""
    idx = np.arange(n_classes, dtype=np.float32)
    y32 = np.float32(2.0) * idx / np.float32(n_classes - 1) - np.float32(1.0)
    return np.linspace(1, 0, 20 * hop), (_fold.decode_mu_law(y32.astype(np.float64), n_classes, False) if mu_law else None)


def chunk_tables_on_device(hop, n_classes, mu_law, device):
    """Make the cached tables `chunk_on_device` reads (tail fade, mu-law expansion) on the CURRENT stream: for a caller whose first launch would
    otherwise create them on a side stream."""
    _fade_tables(0, hop, device)
    if mu_law:
        _mu_law_lut(n_classes, device)


def chunk_on_device(segments, wave_len, t0, t1, hop, n_classes, mu_law, out64=None, out32=None, row=None, min_wave_len=None):
    """One `wrnn_post_chunk` launch on the current stream: steps [t0, t1) of the post-loop stage of unfolded utterances.  segments: float32 CUDA
    (rows, T), the loop's `out`, of which only [t0, t1) need be finished; wave_len: int32 CUDA (n,); row: int32 CUDA (n,) or None (utterance u is
    row u); out64 / out32: float64 / float32 CUDA buffers of at least n * (t1 - t0) elements, at least one of them -- written as [n][t1 - t0].
    Nothing is allocated, nothing synchronises.  The kernel cannot refuse what it reads from the device: the caller vouches that every wave_len is
    >= 20 * hop (`min_wave_len`, the smallest of them, is checked here when given: the reference's ValueError, :258) and every row < segments.shape[0]."""
    dev = segments.device
    if not (segments.is_cuda and segments.dtype == torch.float32 and segments.is_contiguous() and segments.dim() == 2):
        raise ValueError('segments must be a contiguous float32 CUDA tensor (rows, T)')
    n, w = int(wave_len.shape[0]), int(t1) - int(t0)
    if not (wave_len.is_cuda and wave_len.dtype == torch.int32 and wave_len.is_contiguous()) or \
            (row is not None and not (row.is_cuda and row.dtype == torch.int32 and row.is_contiguous() and row.shape == wave_len.shape)):
        raise ValueError('wave_len / row must be contiguous int32 CUDA tensors of one entry per utterance')
    if row is None and n > segments.shape[0]:
        raise ValueError('more utterances than rows of segments')
    if min_wave_len is not None and min_wave_len < 20 * hop:
        raise ValueError(f'operands could not be broadcast together with shapes ({min_wave_len},) ({20 * hop},)')
    for o, dt in ((out64, torch.float64), (out32, torch.float32)):
        if o is not None and not (o.is_cuda and o.dtype == dt and o.is_contiguous() and o.numel() >= n * max(w, 0)):
            raise ValueError('out64 / out32: contiguous CUDA buffers of n * (t1 - t0) float64 / float32 elements')
    _, _, tail = _fade_tables(0, hop, dev)
    lut = _mu_law_lut(n_classes, dev) if mu_law else None
    c = _lib.PostChunkCall(n_utt=n, T=int(segments.shape[1]), t0=int(t0), t1=int(t1), n_classes=int(n_classes), tail_len=20 * hop,
                           segments=segments.data_ptr(), row=None if row is None else row.data_ptr(), wave_len=wave_len.data_ptr(),
                           lut=None if lut is None else lut.data_ptr(), tail=tail.data_ptr(), out64=None if out64 is None else out64.data_ptr(),
                           out32=None if out32 is None else out32.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    rc = L.wrnn_post_chunk(ctypes.byref(c))
    if rc != 0:
        raise _lib.WrnnError(f'wrnn_post_chunk failed (rc={rc}): {L.wrnn_post_last_error().decode()}')
