"""The teacher-forced loop in a chosen precision, and float64 samplers -- TEST INFRASTRUCTURE, never shipped / never measured.

`oracle/wavernn_oracle.py` and `oracle/wrnn_oracle.c` are float32: where they disagree with a kernel nothing says which side is right.  `loop_forced` runs the
steps of `wavernn_oracle.loop` (I -> rnn1 -> rnn2 -> fc1 -> fc2 -> fc3, reference models/fatchord_version.py:203-223) in float64 (the truth), in float32 in the
reference's plain order (what its arithmetic loses), or in float32 with every matrix product summed in chunks of `k_chunk` columns in a seeded permuted order (a
second float32 baseline whose summation order differs the way a kernel's does).  It does no sampling: the fed-back sample is given.

The samplers (`raw_ratios64`, `mol_sample64`) are float64 restatements of `wavernn_oracle.sample_raw` / `sample_mol` on float32 inputs: they say what a float32
sampler may legitimately answer on given logits -- which classes / components are near-ties, and how far from the exact value a sample may land.
"""
import numpy as np

LOG_SCALE_MIN = float(np.log(1e-14))            # `log_scale_min` of utils/distribution.py:87 (-32.236...)
GATE_LO, GATE_HI, N_SAT = 0.02, 0.98, 0.96      # a gate value outside [GATE_LO, GATE_HI], a candidate |n| > N_SAT, counts as saturated

_KEYS = ('I.weight', 'I.bias', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn1.bias_ih_l0', 'rnn1.bias_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0',
         'rnn2.bias_ih_l0', 'rnn2.bias_hh_l0', 'fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias', 'fc3.weight', 'fc3.bias')


class _Product:
    """x -> x @ W.T in `dtype`: numpy's own product (k_chunk None), or partial sums over chunks of `k_chunk` columns, added one after the other in a
    permuted order, every partial sum rounded to `dtype`."""

    def __init__(self, W, dtype, k_chunk, rs):
        self.W = np.ascontiguousarray(W, dtype)
        self.dtype = dtype
        self.chunks = None
        if k_chunk:
            N, K = self.W.shape
            n = -(-K // k_chunk)
            Wp = np.zeros((N, n * k_chunk), dtype)
            Wp[:, :K] = self.W
            self.K, self.k = K, k_chunk
            self.chunks = np.ascontiguousarray(Wp.reshape(N, n, k_chunk).transpose(1, 2, 0))      # [n][k_chunk][N]
            self.order = rs.permutation(n)

    def __call__(self, x):
        if self.chunks is None:
            return (x @ self.W.T).astype(self.dtype)
        B = x.shape[0]
        n = self.chunks.shape[0]
        xp = np.zeros((B, n * self.k), self.dtype)
        xp[:, :self.K] = x
        part = np.matmul(np.ascontiguousarray(xp.reshape(B, n, self.k).transpose(1, 0, 2)), self.chunks).astype(self.dtype)      # [n][B][N]
        acc = part[self.order[0]].copy()
        for i in self.order[1:]:
            acc = (acc + part[i]).astype(self.dtype)
        return acc


def loop_forced(sd, mode, mels, aux, force_x, dtype=np.float64, k_chunk=None, k_seed=None):
    """The loop of `wavernn_oracle.loop` in `dtype`, teacher-forced: mels (B, T, feat), aux (B, T, 4 * aux_dims), force_x (B, T) = the sample fed back
    AFTER step t (`x_t`; step 0 reads 0, as every loop kernel's `force_x` does).  Returns (logits [T, B, C] in `dtype`, stats) with stats =
    {'rnn1': {'r': share, 'z': share, 'n': share}, 'rnn2': ...}: the share of r / z values outside [0.02, 0.98] and of |n| > 0.96 over all steps, segments
    and units.  `mode` names the head only for symmetry with `wavernn_oracle.loop`: nothing is sampled.  dtype=np.float32: the float32 oracle's expressions
    in their order (its logits bit for bit); with k_chunk / k_seed see `_Product`."""
    if mode not in ('MOL', 'RAW'):
        raise RuntimeError("Unknown model mode value - ", mode)
    dt = np.dtype(dtype).type
    rs = np.random.RandomState(k_seed) if k_chunk else None
    w = {}
    for k in _KEYS:                                  # (the order of _KEYS fixes which permutation a matrix gets)
        w[k] = _Product(sd[k], dt, k_chunk, rs) if 'weight' in k else np.ascontiguousarray(sd[k], dt)
    mels, aux, force_x = (np.ascontiguousarray(a, dt) for a in (mels, aux, force_x))
    B, T, _ = mels.shape
    H = w['rnn1.weight_hh_l0'].W.shape[1]
    d = aux.shape[2] // 4
    one = dt(1)
    count = {g: dict(r=0, z=0, n=0) for g in ('rnn1', 'rnn2')}

    def sigmoid(x):
        return (one / (one + np.exp(-x, dtype=dt))).astype(dt)

    def gru(name, x, h):
        # ATen's gru_cell as `wavernn_oracle.gru_cell` restates it
        gi = (w[name + '.weight_ih_l0'](x) + w[name + '.bias_ih_l0']).astype(dt)
        gh = (w[name + '.weight_hh_l0'](h) + w[name + '.bias_hh_l0']).astype(dt)
        r = sigmoid(gh[:, :H] + gi[:, :H])
        z = sigmoid(gh[:, H:2 * H] + gi[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + gh[:, 2 * H:] * r, dtype=dt)
        c = count[name]
        c['r'] += int(np.count_nonzero((r < GATE_LO) | (r > GATE_HI)))
        c['z'] += int(np.count_nonzero((z < GATE_LO) | (z > GATE_HI)))
        c['n'] += int(np.count_nonzero(np.abs(n) > N_SAT))
        return ((h - n) * z + n).astype(dt)

    h1, h2, x = np.zeros((B, H), dt), np.zeros((B, H), dt), np.zeros((B, 1), dt)
    out = []
    with np.errstate(over='ignore'):                 # exp(-x) of a saturated float32 gate is inf, the gate 0: the reference's own arithmetic
        for t in range(T):
            a1, a2, a3, a4 = (aux[:, t, d * k:d * (k + 1)] for k in range(4))
            xx = (w['I.weight'](np.concatenate([x, mels[:, t], a1], axis=1)) + w['I.bias']).astype(dt)
            h1 = gru('rnn1', xx, h1)
            xx = xx + h1
            h2 = gru('rnn2', np.concatenate([xx, a2], axis=1), h2)
            xx = xx + h2
            xx = np.maximum(w['fc1.weight'](np.concatenate([xx, a3], axis=1)) + w['fc1.bias'], 0).astype(dt)
            xx = np.maximum(w['fc2.weight'](np.concatenate([xx, a4], axis=1)) + w['fc2.bias'], 0).astype(dt)
            out.append((w['fc3.weight'](xx) + w['fc3.bias']).astype(dt))
            x = force_x[:, t:t + 1]
    total = float(T * B * H)
    return np.stack(out), {g: {k: v / total for k, v in c.items()} for g, c in count.items()}


def raw_ratios64(logits, q):
    """p / q in float64 in the reference's order (fatchord_version.py:232-235 as `wavernn_oracle.sample_raw` restates it): softmax, renormalise, divide.
    logits, q: (..., C) float32.  The class drawn is the FIRST maximum of the result."""
    lg, q = np.asarray(logits, np.float64), np.asarray(q, np.float64)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    p = p / p.sum(axis=-1, keepdims=True)
    return p / q


def mol_sample64(logits, u1, u2, k=None):
    """`sample_from_discretized_mix_logistic` (utils/distribution.py:87-123) in float64 on float32 inputs, for one step: logits (B, 30), u1 (B, 10), u2 (B,).
    Returns (scores, x, m): the gumbel scores lp - log(-log u1) [B, 10]; for component k (an int array (B,); None: the argmax of the scores) the UNCLIPPED
    x = mean + exp(max(ls, log 1e-14)) (log u2 - log(1 - u2)); and its magnitude m = |mean| + exp(ls) (|log u2| + |log(1 - u2)|), the sum of the sizes of
    the terms a float32 sampler rounds."""
    lg, u1, u2 = np.asarray(logits, np.float64), np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    nr = lg.shape[1] // 3
    scores = lg[:, :nr] - np.log(-np.log(u1))
    if k is None:
        k = np.argmax(scores, axis=1)
    rows = np.arange(lg.shape[0])
    mean = lg[rows, nr + k]
    s = np.exp(np.maximum(lg[rows, 2 * nr + k], LOG_SCALE_MIN))
    a, b = np.log(u2), np.log(1.0 - u2)
    return scores, mean + s * (a - b), np.abs(mean) + s * (np.abs(a) + np.abs(b))
