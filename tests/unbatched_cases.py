"""Inputs shared by tests/test_post_chunk_host.py and tests/test_gpu_unbatched.py: the post-loop stage of a step range (`wrnn_post_chunk`,
`wrnn_post_chunk_host`) on three ragged rows, and the step ranges at which it can go wrong.  Not collected by pytest."""
import numpy as np

HOP, C = 275, 512
TAIL_LEN = 20 * HOP
T = 29 * HOP                                                  # 7975: the longest row, 29 frames
WAVE_LEN = np.array([20 * HOP, 23 * HOP, 28 * HOP], np.int32)   # 5500 (== tail_len: the fade starts at step 0), 6325, 7700


def segments(kind):
    """(rows (3, T) float32, mu_law): 'mol' sample values, 'raw_lut' / 'raw' 9-bit class values 2 idx / (C - 1) - 1 with / without the expansion table."""
    rs = np.random.RandomState({'mol': 41, 'raw_lut': 42, 'raw': 43}[kind])
    if kind == 'mol':
        return rs.uniform(-1, 1, size=(3, T)).astype(np.float32), False
    idx = rs.randint(0, C, size=(3, T)).astype(np.float32)
    idx[:, :4] = [0, C - 1, 1, C - 2]                         # the table's ends
    return (np.float32(2.0) * idx / np.float32(C - 1) - np.float32(1.0)).astype(np.float32), kind == 'raw_lut'


def reference(seg, mu_law, row=None):
    """(3, T) float64: `fold.finish_waveform` of every row (after `decode_mu_law`), zeros past wave_len -- utterance u reads row[u]."""
    from wavernn_amd import fold as F
    out = np.zeros((3, T), np.float64)
    for u in range(3):
        y = seg[u if row is None else int(row[u])].astype(np.float64)
        if mu_law:
            y = F.decode_mu_law(y, C, False)
        out[u, :WAVE_LEN[u]] = F.finish_waveform(y.copy(), int(WAVE_LEN[u]), HOP)
    return out


def cover(k):
    return [(a, min(T, a + k)) for a in range(0, T, k)]


#: name -> list of [t0, t1)
RANGES = {
    'chunks-997': cover(997),                                 # odd, no multiple of 4: every row base row * T + t0 is unaligned
    'chunks-1651': cover(1651),
    'one-chunk': [(0, T)],
    'straddle-fade-start': [(813, 839), (2190, 2211)],        # wave_len - tail_len = 825 (row 1), 2200 (row 2)
    'straddle-wave-len': [(5490, 5513), (6321, 6330), (7699, 7702)],
    'past-a-short-one': [(5600, 6001), (7701, T)],            # wholly past row 0's (and every row's) wave_len
    'fade-from-step-0': [(0, 7), (1, 2)],                     # row 0: wave_len == tail_len
}
ROWS = [None, np.array([2, 0, 1], np.int32)]
