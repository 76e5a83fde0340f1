"""Trained-like weights for the loop kernels, the cases built on them, and the checkers of tests/test_trained_like_host.py (CPU: is a case a valid test
input?) and tests/test_gpu_trained_like.py (GPU: every loop kernel on those cases) -- TEST ONLY.

Why: `synthetic.random_state_dict` draws torch's default initialisers.  Under them no GRU gate leaves the linear part of its activation, the RAW softmax is
almost uniform (largest probability 0.003) and the MoL log-scales sit in -3.2 ... -2.9: the saturating branches of the activations, exp() underflow in the RAW
samplers, the MoL `log_scale_min` clamp and both +-1 clips never run.  `trained_like` scales a state dict into that regime.

How a kernel is held there.  Scaled-up GRU matrices make the loop sensitive to rounding, so neither a fixed tolerance against a float32 oracle nor sample
equality against an oracle trajectory can hold for a correct kernel.  Instead (1) the truth is `oracle.loop_f64.loop_forced` in float64 on a fixed teacher-forced
input; (2) a kernel's logits may be off by K = 8 times what the float32 reference arithmetic itself loses on the same case (E_ref: plain and permuted summation
order, both measured against the float64 run), rounding noise being amplified alike on both sides; (3) the samplers are checked on the kernel's OWN logits --
every loop kernel writes its own sample to `out` before it substitutes `force_x` -- against float64 samplers, near-ties excused (and counted).
"""
import numpy as np

from oracle import loop_f64 as F
from oracle import wavernn_oracle as O

K = 8                                   # a kernel's error bound in units of the float32 reference's own error (logits: E_ref; MoL values: E_samp)
E_REF_MAX = 1e-5                        # a case whose float32 reference is off the float64 one by more is in the chaotic regime: lower its gain
RAW_TIE, MOL_TIE = 1e-4, 1e-5           # near-ties: 1 - second / best of p / q;  best - second of the gumbel scores, relative to 1 + |best|
EXCUSED_MAX = 0.005                     # largest share of near-tie steps
PERM_CHUNK, PERM_SEED = 16, 3           # the permuted-order float32 baseline of loop_forced

MOL_LOG_SCALE_BIASES = (-36.0, -34.0, -10.0, -8.0, -7.0, -6.0, -5.0, -4.0, -3.0, -2.5)
GRU_BIASES = ('rnn1.bias_ih_l0', 'rnn1.bias_hh_l0', 'rnn2.bias_ih_l0', 'rnn2.bias_hh_l0')


def trained_like(sd, mode, gate_gain, mix_gain=None, seed=1):
    """A copy of state dict `sd` (numpy arrays) in the regime of a trained checkpoint: the four GRU matrices times gate_gain and U(-gate_gain / 2, gate_gain / 2)
    added to the four GRU bias vectors (saturated gates); RAW: fc3.weight times 4 gate_gain (peaked logits); MoL: the mixture rows of fc3.weight times mix_gain
    (a dominant component now and then), the mean rows times gate_gain / 2 and means biased over (-1.1, 1.1) (both clips), the log-scale rows times gate_gain
    with biases from -36 (below the log 1e-14 clamp) to -2.5."""
    f32 = np.float32
    rs = np.random.RandomState(seed)
    out = dict(sd)
    for g in ('rnn1', 'rnn2'):
        for k in ('weight_ih_l0', 'weight_hh_l0'):
            out[f'{g}.{k}'] = (np.asarray(sd[f'{g}.{k}'], f32) * f32(gate_gain)).astype(f32)
    for k in GRU_BIASES:
        b = np.asarray(sd[k], f32)
        out[k] = (b + rs.uniform(-gate_gain / 2.0, gate_gain / 2.0, b.shape).astype(f32)).astype(f32)
    W, b = np.asarray(sd['fc3.weight'], f32).copy(), np.asarray(sd['fc3.bias'], f32).copy()
    if mode == 'RAW':
        W *= f32(4 * gate_gain)
    else:
        W[:10] *= f32(mix_gain)
        W[10:20] *= f32(gate_gain / 2.0)
        W[20:30] *= f32(gate_gain)
        b[:10] = 0
        b[10:20] = rs.permutation(np.linspace(-1.1, 1.1, 10)).astype(f32)
        b[20:30] = rs.permutation(np.array(MOL_LOG_SCALE_BIASES)).astype(f32)
    out['fc3.weight'], out['fc3.bias'] = W, b
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------
#: shipped dims: conditioning as tests/test_gpu_parity.py builds it (the oracle's up-sampling network on a random mel), 40 segments of 64 steps, 40 apart
SHIP = dict(wseed=11, mseed=12, nseed=13, frames=6, B=40, T=64, stride=40, hop=275)
#: other dims: inputs as tests/test_gpu_fallback_dims.py builds them (weights 5 behind a small up-sampling network, uniform conditioning, the even table)
DIMS = dict(wseed=5, mseed=1, nseed=7, T=48, stride=21, hop=8)
D256 = dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128, B=18)
D144 = dict(mode='RAW', rnn_dims=144, fc_dims=80, bits=10, feat_dims=13, res_out_dims=20, B=17)

#: name -> the model (hp: None = shipped), how it is made (prune = (sparsity, linear) BEFORE the recipe, bf16 = rounded AFTER it) and the recipe's gains.
#: Gains start from 6 / 6; a pruned pack needs more (its sums have fewer terms), and where fc1 / fc2 are pruned too a RAW head needs much more.  seed (of the
#: recipe's biases), wseed (weights) and nseed (noise) are chosen so that the conditions of tests/test_trained_like_host.py hold;
#: they are inputs, not tolerances.
CASES = {
    'ship_mol': dict(hp=None, mode='MOL', gate_gain=6, mix_gain=6),
    'ship_raw': dict(hp=None, mode='RAW', gate_gain=7.5, seed=5),
    'ship_pruned_mol': dict(hp=None, mode='MOL', prune=(0.95, True), gate_gain=12, mix_gain=6),
    'ship_pruned_raw': dict(hp=None, mode='RAW', prune=(0.95, True), gate_gain=60, seed=7, wseed=14),
    'd256_mol': dict(hp=D256, gate_gain=6, mix_gain=6),
    'd256_mol_bf16': dict(hp=D256, bf16=True, gate_gain=6, mix_gain=6),
    'd256_mol_pruned': dict(hp=D256, prune=(0.90, True), gate_gain=12, mix_gain=6),
    'd144_raw': dict(hp=D144, gate_gain=7, seed=6),
    'd144_raw_bf16': dict(hp=D144, bf16=True, gate_gain=7, seed=6),
    'd144_raw_pruned': dict(hp=D144, prune=(0.75, True), gate_gain=14, seed=5, wseed=6),
    'g520_raw': dict(hp=dict(mode='RAW', rnn_dims=520, fc_dims=257, bits=10, feat_dims=13, res_out_dims=20, B=4), gate_gain=6, seed=40, wseed=9, nseed=11),
    'g100_raw1': dict(hp=dict(mode='RAW', rnn_dims=100, fc_dims=50, bits=1, feat_dims=7, res_out_dims=4, B=5), gate_gain=6),
}
HP = ('mode', 'rnn_dims', 'fc_dims', 'bits', 'feat_dims', 'res_out_dims')
_MEMO = {}


def base_weights(name):
    """The state dict of a case BEFORE the recipe (pruned where the case says so); memoised, never written to."""
    key = ('base', name)
    if key not in _MEMO:
        from wavernn_amd.prune import block_prune_state_dict
        from wavernn_amd.synthetic import random_state_dict
        cfg = CASES[name]
        if cfg['hp'] is None:
            sd = random_state_dict(cfg.get('wseed', SHIP['wseed']), mode=cfg['mode'])
        else:
            sd = random_state_dict(cfg.get('wseed', DIMS['wseed']), compute_dims=8, res_blocks=1, **{k: cfg['hp'][k] for k in HP})
        if cfg.get('prune'):
            sd, _ = block_prune_state_dict(sd, cfg['prune'][0], (16, 1), linear=cfg['prune'][1])
        _MEMO[key] = sd
    return _MEMO[key]


def weights(name):
    """The model of a case, for the kernel and the oracle alike."""
    key = ('sd', name)
    if key not in _MEMO:
        from wavernn_amd.synthetic import bf16_round_state_dict
        cfg = CASES[name]
        mode = cfg['mode'] if cfg['hp'] is None else cfg['hp']['mode']
        sd = trained_like(base_weights(name), mode, cfg['gate_gain'], cfg.get('mix_gain'), seed=cfg.get('seed', 1))
        _MEMO[key] = bf16_round_state_dict(sd) if cfg.get('bf16') else sd
    return _MEMO[key]


def gather(mels_up, aux, seg_pos, seg_lim, T, hop):
    """The gather every loop kernel does: step t of segment b reads position seg_pos[b] + t and its frame's aux row, zeros from seg_lim[b] on."""
    B = len(seg_pos)
    mels_f, aux_f = np.zeros((B, T, mels_up.shape[1]), np.float32), np.zeros((B, T, aux.shape[1]), np.float32)
    for b in range(B):
        p = int(seg_pos[b]) + np.arange(T)
        ok = p < int(seg_lim[b])
        mels_f[b, ok] = mels_up[p[ok]]
        aux_f[b, ok] = aux[p[ok] // hop]
    return mels_f, aux_f


def inputs(name, T=None):
    """Weights, conditioning, segment table and seeded noise of a case (memoised, never written to): dict(sd, mode, C, B, T, hop, seg_pos, seg_lim, mels_up,
    aux, mels_f, aux_f, noise -- (u1 [T, B, 10], u2 [T, B]) or q [T, B, C] --, flat -- the noise in the launch layout).  T: another number of steps than the
    case's own (the free-running comparisons run 64 at every dims): conditioning and noise are drawn for that length."""
    key = ('in', name, T)
    if key in _MEMO:
        return _MEMO[key]
    from wavernn_amd.synthetic import random_mel
    cfg, sd = CASES[name], weights(name)
    n_classes = sd['fc3.weight'].shape[0]
    if cfg['hp'] is None:
        mode, (B, T0, stride, hop) = cfg['mode'], (SHIP[k] for k in ('B', 'T', 'stride', 'hop'))
        T = T or T0
        m = O.pad_tensor(random_mel(SHIP['mseed'], SHIP['frames']).T[None], 2, 'both')[0].T
        mels_up, aux_up = O.upsample_network(sd, m)
        aux = np.ascontiguousarray(aux_up[::hop])
        L = mels_up.shape[0]
        assert (B - 1) * stride + T <= L
        noise = O.draw_noise(cfg.get('nseed', SHIP['nseed']), mode, B, T)
    else:
        hp = cfg['hp']
        mode, B, (T0, stride, hop) = hp['mode'], hp['B'], (DIMS[k] for k in ('T', 'stride', 'hop'))
        T = T or T0
        A = hp['res_out_dims'] // 4
        L = -(-((B - 1) * stride + T) // hop) * hop
        rs = np.random.RandomState(DIMS['mseed'])
        mels_up = rs.uniform(0, 1, (L, hp['feat_dims'])).astype(np.float32)
        aux = rs.uniform(-1, 1, (L // hop, 4 * A)).astype(np.float32)
        noise = O.draw_noise(cfg.get('nseed', DIMS['nseed']), mode, B, T, rnn_dims=hp['rnn_dims'], aux_dims=A, n_classes=n_classes)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * np.int32(stride), np.full(B, L, np.int32)
    mels_f, aux_f = gather(mels_up, aux, seg_pos, seg_lim, T, hop)
    if mode == 'MOL':
        noise = tuple(np.ascontiguousarray(n, np.float32) for n in noise)
        flat = np.ascontiguousarray(np.concatenate([noise[0].reshape(T, B * 10), noise[1].reshape(T, B)], axis=1))
    else:
        noise = flat = np.ascontiguousarray(noise, np.float32)
    _MEMO[key] = dict(name=name, sd=sd, mode=mode, C=n_classes, B=B, T=T, hop=hop, stride=stride, seg_pos=seg_pos, seg_lim=seg_lim, mels_up=mels_up, aux=aux,
                      mels_f=mels_f, aux_f=aux_f, noise=noise, flat=flat)
    return _MEMO[key]


def rel_logit_error(L, L64):
    """max over (t, b, c) of |L - L64| / (1 + max_c |L64[t, b, :]|)."""
    L64 = np.asarray(L64, np.float64)
    return float((np.abs(np.asarray(L, np.float64) - L64) / (1.0 + np.abs(L64).max(axis=2, keepdims=True))).max())


def case(name):
    """`inputs(name)` plus everything the oracle says about the case, each run done once (memoised, never written to): force_x [B, T] = the float32 oracle's
    own free run on these weights and this noise; L64, gates = the float64 teacher-forced run and its gate statistics; L32 / L32p = the float32 runs in
    plain / permuted order; e_ref; MoL: e_samp = max |x32 - clip(x64)| / m of `wavernn_oracle.sample_mol` on L32."""
    key = ('case', name)
    if key in _MEMO:
        return _MEMO[key]
    c = dict(inputs(name))
    sd, mode, args = c['sd'], c['mode'], (c['mels_f'], c['aux_f'])
    c['force_x'] = O.loop(sd, mode, *args, c['noise'])
    c['L64'], c['gates'] = F.loop_forced(sd, mode, *args, c['force_x'])
    c['L32'], _ = F.loop_forced(sd, mode, *args, c['force_x'], dtype=np.float32)
    c['L32p'], _ = F.loop_forced(sd, mode, *args, c['force_x'], dtype=np.float32, k_chunk=PERM_CHUNK, k_seed=PERM_SEED)
    c['e_plain'], c['e_perm'] = rel_logit_error(c['L32'], c['L64']), rel_logit_error(c['L32p'], c['L64'])
    c['e_ref'] = max(c['e_plain'], c['e_perm'])
    if mode == 'MOL':
        e = 0.0
        for t in range(c['T']):
            x32, k = O.sample_mol(c['L32'][t], c['noise'][0][t], c['noise'][1][t])
            _, x64, m = F.mol_sample64(c['L32'][t], c['noise'][0][t], c['noise'][1][t], k)
            e = max(e, float((np.abs(x32.astype(np.float64) - np.clip(x64, -1, 1)) / m).max()))
        c['e_samp'] = e
    _MEMO[key] = c
    return c


# ---- what a set of logits does to the samplers (float64, on float32 logits and the case's noise) ----------------------------------------------------------
def raw_profile(L, q):
    """RAW logits [T, B, C], noise q [T, B, C] -> dict: pmax [T, B] the softmax maximum; first / second [T, B] the two best classes of the float64 p / q
    (an exact tie: the lower index first, the first-maximum rule); near [T, B]: 1 - second / best < RAW_TIE; exact [T, B]: the two best ratios are equal."""
    r = F.raw_ratios64(L, q)
    lg = np.asarray(L, np.float64)
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    order = np.argsort(-r, axis=2, kind='stable')[:, :, :2]             # (stable: equal ratios stay in index order)
    best, second = np.take_along_axis(r, order[:, :, :1], 2)[:, :, 0], np.take_along_axis(r, order[:, :, 1:2], 2)[:, :, 0]
    return dict(pmax=(e / e.sum(axis=2, keepdims=True)).max(axis=2), first=order[:, :, 0], second=order[:, :, 1], near=(1.0 - second / best) < RAW_TIE,
                exact=second == best)


def mol_profile(L, u1, u2):
    """MoL logits [T, B, 30], noise u1 [T, B, 10], u2 [T, B] -> dict: first / second [T, B] the two best components of the float64 gumbel scores; near
    [T, B]: best - second < MOL_TIE (1 + |best|); x / m (and x2 / m2 for the second-best component): `mol_sample64`; ls [T, B] the chosen log-scale."""
    T, B = u2.shape
    out = {k: np.zeros((T, B)) for k in ('x', 'm', 'x2', 'm2', 'ls')}
    out.update(first=np.zeros((T, B), np.int64), second=np.zeros((T, B), np.int64), near=np.zeros((T, B), bool))
    rows = np.arange(B)
    for t in range(T):
        s, x, m = F.mol_sample64(L[t], u1[t], u2[t])
        order = np.argsort(-s, axis=1, kind='stable')
        k1, k2 = order[:, 0], order[:, 1]
        _, x2, m2 = F.mol_sample64(L[t], u1[t], u2[t], k2)
        best, second = s[rows, k1], s[rows, k2]
        out['first'][t], out['second'][t], out['near'][t] = k1, k2, (best - second) < MOL_TIE * (1.0 + np.abs(best))
        out['x'][t], out['m'][t], out['x2'][t], out['m2'][t] = x, m, x2, m2
        out['ls'][t] = np.asarray(L[t], np.float64)[rows, 20 + k1]
    return out


# ---- the checkers: assertions 1-4 on one call's (out [B, T], logits [T, B, C]) -----------------------------------------------------------------------
def check_finite(out, Lk, what):
    assert np.isfinite(Lk).all(), f'{what}: {np.count_nonzero(~np.isfinite(Lk))} logits are not finite'
    assert np.isfinite(out).all(), f'{what}: {np.count_nonzero(~np.isfinite(out))} samples are not finite'


def check_logits(Lk, c, what):
    """Assertion 2: max |Lk - L64| / (1 + max_c |L64|) <= K E_ref, E_ref from the case's own float32 runs.  Returns the error."""
    assert Lk.shape == c['L64'].shape, (what, Lk.shape)
    err = rel_logit_error(Lk, c['L64'])
    print(f"{what}: E_ref = {c['e_ref']:.3e}, logits off float64 by {err:.3e} = {err / c['e_ref']:.2f} E_ref")
    assert err <= K * c['e_ref'], f"{what}: logits off the float64 loop by {err:.3e} = {err / c['e_ref']:.2f} E_ref (bound {K} E_ref, E_ref = {c['e_ref']:.3e})"
    return err


def check_raw(out, Lk, q, what):
    """Assertion 3: `out` [B, T] against the RAW sampler on the kernel's own logits Lk [T, B, C].  Away from near-ties out == `wavernn_oracle.sample_raw(Lk[t],
    q[t])`, value for value; at an EXACT tie of the two best float64 ratios (equal logits and equal noise: every float32 sampler forms equal ratios too) the
    first-maximum rule decides, the lower class; at any other near-tie either of the two best classes, as its exact grid value.  Returns the near-tie share."""
    T, B, C = Lk.shape
    p = raw_profile(Lk, q)
    got = np.ascontiguousarray(out.T)
    grid = lambda idx: (np.float32(2) * idx.astype(np.float32) / np.float32(C - 1.) - np.float32(1.)).astype(np.float32)
    want = np.stack([O.sample_raw(Lk[t], q[t])[0] for t in range(T)])
    excusable = p['near'] & ~p['exact']
    ok = np.where(excusable, (got == grid(p['first'])) | (got == grid(p['second'])), np.where(p['exact'], got == grid(p['first']), got == want))
    bad = np.argwhere(~ok)
    assert bad.size == 0, (f'{what}: {len(bad)} of {T * B} samples are not the class the RAW sampler draws from the kernel\'s own logits, first at (step, segment) = '
                           f'{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}')
    share = float(excusable.mean())
    assert share <= EXCUSED_MAX, f'{what}: {share:.4f} of the steps are RAW near-ties'
    return share


def check_mol(out, Lk, u1, u2, e_samp, what):
    """Assertion 4: `out` [B, T] against the float64 MoL sampler on the kernel's own logits Lk [T, B, 30]: |out - clip(x64, -1, 1)| <= K e_samp m with the
    float64 argmax component (at a gumbel near-tie: or with the second-best); a sample whose x64 lies beyond +-1 by more than that is exactly +-1.  Returns
    dict(near, clamp, lo, hi): the near-tie share and the number of steps that ran the log-scale clamp, the -1 clip and the +1 clip -- each asserted > 0."""
    T, B, _ = Lk.shape
    p = mol_profile(Lk, u1, u2)
    got = np.ascontiguousarray(out.T).astype(np.float64)

    def fits(x, m):
        tol = K * e_samp * m
        return (np.abs(got - np.clip(x, -1, 1)) <= tol) & ((x <= 1 + tol) | (got == 1.0)) & ((x >= -1 - tol) | (got == -1.0))

    ok = fits(p['x'], p['m']) | (p['near'] & fits(p['x2'], p['m2']))
    bad = np.argwhere(~ok)
    if bad.size:
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {T * B} samples are off the float64 MoL sampler on the kernel's own logits, first at (step, segment) = {i}: "
                             f"got {got[i]!r}, x64 {p['x'][i]!r} (component {p['first'][i]}, log-scale {p['ls'][i]:.3f}), "
                             f"|diff| / m = {abs(got[i] - np.clip(p['x'][i], -1, 1)) / p['m'][i]:.3e}, bound {K * e_samp:.3e}")
    res = dict(near=float(p['near'].mean()), clamp=int(np.count_nonzero(p['ls'] < F.LOG_SCALE_MIN)), lo=int(np.count_nonzero(p['x'] < -1)),
               hi=int(np.count_nonzero(p['x'] > 1)))
    assert res['near'] <= EXCUSED_MAX, f"{what}: {res['near']:.4f} of the steps are gumbel near-ties"
    assert res['clamp'] > 0 and res['lo'] > 0 and res['hi'] > 0, f'{what}: the clamp / -1 clip / +1 clip ran at {res} steps: one of them never'
    return res


def check_call(out, Lk, c, what):
    """Assertions 1-4 on one teacher-forced call of a kernel on case `c`."""
    check_finite(out, Lk, what)
    check_logits(Lk, c, what)
    if c['mode'] == 'RAW':
        return check_raw(out, Lk, c['noise'], what)
    return check_mol(out, Lk, c['noise'][0], c['noise'][1], c['e_samp'], what)
