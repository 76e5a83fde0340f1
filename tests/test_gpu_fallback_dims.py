"""The two fallback loop kernels at the dimension and class-count edges: `wrnn_generic_kernel` (csrc/wrnn_generic.hip: any rnn / fc / feat / aux dims and
RAW class count) and `wrnn_stream_kernel` (csrc/wrnn_stream.hip: the shipped dims with a RAW class count other than 512).  tests/test_gpu_parity.py and
tests/test_gpu_noise.py reach them at one geometry (rnn 256, fc 384, 8 bits, feat 40, aux 16) in which every dim is a multiple of 64 and H, F, C are below
the 512-thread workgroup; here every case is chosen for a piece of code that geometry never runs:

    id  mode  rnn   fc   classes  feat  aux   kernel    what it reaches
    G1  RAW   520   257  1024     13    5     generic   H one row past a stride of the row loops; odd F; keep[1]; K0 = 19
    G2  RAW   72    600  2048     80    32    generic   F > H (HF from F, a2 / a4 at different offsets of `va`); F past a stride; all four keep[] slots
    G3  RAW   100   50   2        7     1     generic   the smallest C, A = 1, less than one wave of everything
    G4  MOL   1030  33   30       3     3     generic   three trips of the H loops, F below a wave
    S1  RAW   512   512  256      80    32    stream    half the lanes carry -inf through the sampler's reductions
    S2  RAW   512   512  32       80    32    stream    seven empty waves
    S3  RAW   512   512  2        80    32    stream    two classes
    S4  RAW   512   512  1024     80    32    generic   the shipped dims with more classes than the stream kernel has threads

Two references.  The C oracle (oracle/wrnn_oracle.c) gives the sampled trajectory and float32 logits; `_f64_logits` below, a plain float64 numpy restatement
of fatchord_version.py:203-223 teacher-forced with the oracle's samples, gives the logits every float32 implementation is measured against.  The bound on
the kernel's teacher-forced logits is K * E_ref with E_ref = max|oracle float32 logits - float64 logits| of the same case: it comes from the reference side
alone.  K = 8: another float32 summation order over at most 2100 terms stays within a small multiple of E_ref (the oracle's own rounding error) -- see
`test_teacher_forced_logits` for what was measured.

The inputs are guarded on the CPU before anything is launched (`_guards`): no segment-step of a RAW case is a near-tie (the `_tie` criterion of
tests/test_gpu_sparse_raw.py: float64 p / q, relative gap <= 1e-6), so class indices can be demanded EQUAL without excusing anything; and zeroing the last
input column of any of the eight matrices -- the term a wrong loop bound or stride would drop -- moves the float64 logits by at least 50 * K * E_ref, so the
bound tells such a kernel from a right one.

Seeds: weights 5 (see WSEED), mel / aux 1, noise 7."""
import numpy as np
import pytest
import torch

from helpers import MOL_TOL

pytestmark = pytest.mark.gpu

T = 64
HOP, STRIDE = 8, 21                # the even table: segment b starts at 21 b (no multiple of the hop), every step live
RAGGED_HOP = 7
MSEED, NSEED = 1, 7
#: weight seed (of `random_state_dict`, drawn behind a small up-sampling network: compute_dims 8, one res block -- the loop never reads it, but its size
#: moves the stream the loop weights come from).  The discrimination guard needs every "last input column" to matter; a seed can fail it -- when the
#: last unit of y2 is dead under the ReLU at every step, zeroing fc3's last column moves nothing and a kernel that dropped it would pass.  With 5, all
#: eight mutants of all eight cases and of the two ragged tables clear 50 * K * E_ref (<= 9.7e-5): the weakest moves the logits by 5.3e-4 (G4 ragged,
#: rnn2.weight_hh), and no RAW step is a near-tie.  `_guards` asserts both, so another seed cannot weaken the tests quietly.
WSEED = 5
K = 8                              # logits bound = K * E_ref (see the module docstring); never above TF_BAR
TF_BAR = 1e-4                      # the project's teacher-forced bar (tests/test_gpu_parity.py)
TIE_REL = 1e-6
LIB_SEED = 0x5EED0123456789AB

GENERIC, STREAM = 'wrnn_generic_kernel', 'wrnn_stream_kernel'
CASES = {
    'G1': dict(mode='RAW', rnn_dims=520, fc_dims=257, bits=10, feat_dims=13, res_out_dims=20, B=4, kernel=GENERIC),
    'G2': dict(mode='RAW', rnn_dims=72, fc_dims=600, bits=11, feat_dims=80, res_out_dims=128, B=3, kernel=GENERIC),
    'G3': dict(mode='RAW', rnn_dims=100, fc_dims=50, bits=1, feat_dims=7, res_out_dims=4, B=5, kernel=GENERIC),
    'G4': dict(mode='MOL', rnn_dims=1030, fc_dims=33, bits=9, feat_dims=3, res_out_dims=12, B=3, kernel=GENERIC),
    'S1': dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=8, feat_dims=80, res_out_dims=128, B=4, kernel=STREAM),
    'S2': dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=5, feat_dims=80, res_out_dims=128, B=4, kernel=STREAM),
    'S3': dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=1, feat_dims=80, res_out_dims=128, B=4, kernel=STREAM),
    'S4': dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=10, feat_dims=80, res_out_dims=128, B=3, kernel=GENERIC),
}
MATRICES = ('I.weight', 'rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0', 'fc1.weight', 'fc2.weight', 'fc3.weight')
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


# ---- the references (CPU) --------------------------------------------------------------------------------------------------------------------
def _f64_logits(sd, mels, aux, x_fed):
    """fatchord_version.py:203-223 in float64, teacher-forced: mels [B, T, M], aux [B, T, 4 A], x_fed [B, T] = the sample fed back AFTER step t (step 0
    reads 0).  Returns the logits [T, B, C]."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items() if k.split('.')[0] in ('I', 'rnn1', 'rnn2', 'fc1', 'fc2', 'fc3')}
    mels, aux, x_fed = (np.asarray(a, np.float64) for a in (mels, aux, x_fed))
    B, steps, _ = mels.shape
    H, A = w['rnn1.weight_hh_l0'].shape[1], aux.shape[2] // 4
    a1, a2, a3, a4 = (aux[:, :, i * A:(i + 1) * A] for i in range(4))

    def gru(name, x, h):
        gi = x @ w[name + '.weight_ih_l0'].T + w[name + '.bias_ih_l0']
        gh = h @ w[name + '.weight_hh_l0'].T + w[name + '.bias_hh_l0']
        r = 1.0 / (1.0 + np.exp(-(gi[:, :H] + gh[:, :H])))
        z = 1.0 / (1.0 + np.exp(-(gi[:, H:2 * H] + gh[:, H:2 * H])))
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1.0 - z) * n + z * h

    h1, h2, x = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, 1))
    out = []
    for t in range(steps):
        v = np.concatenate([x, mels[:, t], a1[:, t]], axis=1) @ w['I.weight'].T + w['I.bias']
        h1 = gru('rnn1', v, h1)
        v = v + h1
        h2 = gru('rnn2', np.concatenate([v, a2[:, t]], axis=1), h2)
        v = v + h2
        v = np.maximum(np.concatenate([v, a3[:, t]], axis=1) @ w['fc1.weight'].T + w['fc1.bias'], 0.0)
        v = np.maximum(np.concatenate([v, a4[:, t]], axis=1) @ w['fc2.weight'].T + w['fc2.bias'], 0.0)
        out.append(v @ w['fc3.weight'].T + w['fc3.bias'])
        x = x_fed[:, t:t + 1]
    return np.stack(out)


def _tie(logits, q):
    """fatchord_version.py:231-237 in float64 on one segment-step: True when the two largest p / q are within a relative TIE_REL."""
    lg = np.asarray(logits, np.float64)
    p = np.exp(lg - lg.max())
    p /= p.sum()
    r = np.sort(p / np.asarray(q, np.float64))
    return (r[-1] - r[-2]) <= TIE_REL * r[-1]


def _table(name, table):
    """(hop, seg_pos, seg_lim, L) of a case.  'even': B segments STRIDE apart, all steps live.  'ragged': two utterances of 13 and 15 frames laid end to
    end (hop 7: 91 + 105 positions); segment 1 runs out of the first utterance after 46 of its 64 steps, segment 2 starts at the second utterance's
    offset, segment 3 runs out of the second after 55 steps; positions 45 and 141 are no multiples of the hop."""
    if table == 'ragged':
        return RAGGED_HOP, np.array([0, 45, 91, 141], np.int32), np.array([91, 91, 196, 196], np.int32), 196
    B = CASES[name]['B']
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    return HOP, np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32), L


def _case(name, table='even'):
    """Everything the CPU knows about a case (memoised; nothing here is written to afterwards): weights, conditioning, segment table, noise, the C oracle's
    free run (samples + float32 logits), the float64 logits teacher-forced with those samples, E_ref, the near-tie count and what each of the eight
    last-column mutants moves."""
    key = (name, table)
    if key in _MEMO:
        return _MEMO[key]
    from oracle import c_oracle as C, wavernn_oracle as O
    from wavernn_amd.synthetic import random_state_dict
    cfg = CASES[name]
    mode, H, M, A = cfg['mode'], cfg['rnn_dims'], cfg['feat_dims'], cfg['res_out_dims'] // 4
    sd = random_state_dict(WSEED, compute_dims=8, res_blocks=1, **{k: cfg[k] for k in ('mode', 'rnn_dims', 'fc_dims', 'bits', 'feat_dims', 'res_out_dims')})
    n_classes = sd['fc3.weight'].shape[0]
    hop, seg_pos, seg_lim, L = _table(name, table)
    B = len(seg_pos)
    rs = np.random.RandomState(MSEED)
    mels_up = rs.uniform(0, 1, (L, M)).astype(np.float32)
    aux = rs.uniform(-1, 1, (L // hop, 4 * A)).astype(np.float32)
    # the gather the kernels do: position seg_pos[b] + t, its frame's aux row, zeros from seg_lim[b] on
    mels_f, aux_f = np.zeros((B, T, M), np.float32), np.zeros((B, T, 4 * A), np.float32)
    for b in range(B):
        p = int(seg_pos[b]) + np.arange(T)
        ok = p < int(seg_lim[b])
        mels_f[b, ok] = mels_up[p[ok]]
        aux_f[b, ok] = aux[p[ok] // hop]
    noise = O.draw_noise(NSEED, mode, B, T, rnn_dims=H, aux_dims=A, n_classes=n_classes)
    if mode == 'MOL':
        noise = tuple(np.ascontiguousarray(n, np.float32) for n in noise)
        flat = np.concatenate([noise[0].reshape(T, B * 10), noise[1].reshape(T, B)], axis=1)
    else:
        noise = flat = np.ascontiguousarray(noise, np.float32)
    ref, ref_logits = C.loop(sd, mode, mels_f, aux_f, noise, want_logits=True)
    lg64 = _f64_logits(sd, mels_f, aux_f, ref)
    e_ref = float(np.abs(ref_logits - lg64).max())
    ties = 0 if mode == 'MOL' else sum(bool(_tie(ref_logits[t, b], noise[t, b])) for t in range(T) for b in range(B))
    moved = {}
    for m in MATRICES:
        mutant = dict(sd)
        mutant[m] = sd[m].copy()
        mutant[m][:, -1] = 0
        moved[m] = float(np.abs(_f64_logits(mutant, mels_f, aux_f, ref) - lg64).max())
    _MEMO[key] = dict(cfg=cfg, sd=sd, mode=mode, C=n_classes, B=B, hop=hop, seg_pos=seg_pos, seg_lim=seg_lim, mels_up=mels_up, aux=aux, flat=flat,
                      ref=ref, ref_logits=ref_logits, lg64=lg64, e_ref=e_ref, ties=ties, moved=moved)
    return _MEMO[key]


def _guards(c, name):
    """The guards on the inputs (CPU): the bound is one, no RAW step is a near-tie, every last-column mutant is far outside the bound."""
    bound = K * c['e_ref']
    assert 0 < bound <= TF_BAR, (name, c['e_ref'])
    assert c['ties'] == 0, f"{name}: {c['ties']} segment-steps of the oracle's run are near-ties"
    weak = {m: d for m, d in c['moved'].items() if d < 50 * bound}
    assert not weak, f'{name}: zeroing the last input column moves the float64 logits by less than 50 K E_ref = {50 * bound:.2e}: {weak}'
    return bound


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def _engine(gpu, name):
    if ('engine', name) not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        _MEMO[('engine', name)] = LoopEngine(_case(name)['sd'], CASES[name]['mode'], device=gpu)
    return _MEMO[('engine', name)]


def _run(gpu, name, table='even', forced=False, noise='oracle', **kw):
    """One `run_segments` call of a case on its table; forced: fed the oracle's samples, returns (samples, logits), else the samples."""
    c, eng = _case(name, table), _engine(gpu, name)
    key = ('dev', name, table)
    if key not in _MEMO:
        _MEMO[key] = tuple(torch.from_numpy(c[k]).to(gpu) for k in ('mels_up', 'aux', 'flat', 'ref'))
    mels_up, aux, flat, ref = _MEMO[key]
    if forced:
        kw.update(force_x=ref, want_logits=True)
    res = eng.run_segments(mels_up, aux, c['seg_pos'], c['seg_lim'], T, flat if noise == 'oracle' else noise, c['hop'], **kw)
    assert eng.last_loop_kernel() == CASES[name]['kernel'], (name, eng.last_loop_kernel())
    return tuple(r.cpu().numpy() for r in res) if forced else res.cpu().numpy()


def _check_samples(c, name, out, what):
    if c['mode'] == 'MOL':
        err = float(np.abs(out - c['ref']).max())
        assert err <= MOL_TOL, f'{name} {what}: max|hip - oracle| = {err:.3e}'
    else:
        half = (c['C'] - 1) / 2.0
        got, want = np.rint((out.astype(np.float64) + 1.0) * half).astype(np.int64), np.rint((c['ref'].astype(np.float64) + 1.0) * half).astype(np.int64)
        bad = np.argwhere(got != want)
        assert bad.size == 0 and np.array_equal(out, c['ref']), \
            f'{name} {what}: {len(bad)} of {out.size} class indices differ from the oracle, first at (segment, step) = {tuple(bad[0]) if len(bad) else None}'


def _check_forced(gpu, name, table):
    c = _case(name, table)
    bound = _guards(c, name)
    out, logits = _run(gpu, name, table, forced=True)
    assert logits.shape == c['lg64'].shape and np.isfinite(logits).all()
    err = float(np.abs(logits - c['lg64']).max())
    print(f"{name} {table}: E_ref = {c['e_ref']:.3e}, max|hip - float64| = {err:.3e}, err / E_ref = {err / c['e_ref']:.2f}, "
          f"weakest mutant moves {min(c['moved'].values()):.2e}")
    assert err <= bound, f"{name} {table}: teacher-forced logits off the float64 reference by {err:.3e} = {err / c['e_ref']:.2f} E_ref (bound {K} E_ref)"
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name', list(CASES))
def test_teacher_forced_logits_and_samples(gpu, name):
    """Fed the oracle's samples, every step's logits stay within K * E_ref of the float64 reference, and the samples drawn from them are the oracle's
    (RAW: the same class index at every (segment, step); MoL: within MOL_TOL).

    Measured on an MI355X with K = 8 in force (err = max|hip - float64|; no case is above 4, so K stays 8):
        case   E_ref      err        err / E_ref   weakest mutant moves
        G1     1.53e-07   1.62e-07   1.06          1.50e-03
        G2     1.89e-07   2.19e-07   1.16          4.79e-03
        G3     4.27e-08   3.58e-08   0.84          1.19e-03
        G4     2.41e-07   3.16e-07   1.31          6.82e-04
        S1     1.75e-07   1.49e-07   0.85          1.26e-03
        S2     1.19e-07   1.37e-07   1.15          1.22e-03
        S3     8.77e-08   9.88e-08   1.13          7.39e-04
        S4     1.72e-07   1.75e-07   1.02          1.42e-03"""
    _check_forced(gpu, name, 'even')


@pytest.mark.parametrize('name', list(CASES))
def test_free_run(gpu, name):
    """No force_x: the kernel feeds its own samples back and must walk the oracle's trajectory."""
    c = _case(name)
    _guards(c, name)
    _check_samples(c, name, _run(gpu, name), 'free run')


@pytest.mark.parametrize('name', ['G1', 'G4'])
def test_ragged_segment_table_on_the_generic_kernel(gpu, name):
    """The generic kernel's own segment-table handling (`live = p < lim`, the zero padding past an utterance, `aux + (p / hop) * 4 A`) on the 'ragged'
    table of `_table`: two utterances end to end, hop 7, two segments that run out of their utterance mid-way, one that starts at the second one's offset.

    Measured on an MI355X with K = 8 in force: G1 E_ref 1.47e-07, err 1.77e-07, err / E_ref 1.21 (weakest mutant 1.60e-03); G4 E_ref 2.15e-07,
    err 2.10e-07, err / E_ref 0.98 (weakest mutant 5.35e-04)."""
    _check_forced(gpu, name, 'ragged')
    _check_samples(_case(name, 'ragged'), name, _run(gpu, name, 'ragged'), 'free run')


@pytest.mark.parametrize('name', ['G1', 'G3'])
def test_library_noise_at_the_new_class_counts(gpu, name):
    """The library's own noise at 1024 classes and at 2 (tests/test_gpu_noise.py stops at 256 on this kernel): the run that draws it inside the call equals,
    sample for sample, the run fed `rng.library_noise`'s tensor."""
    from wavernn_amd.rng import library_noise
    c = _case(name)
    ids = (np.arange(c['B'], dtype=np.uint64)[::-1] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF0000000000)
    tensor = library_noise(c['mode'], c['B'], 0, T, c['C'], gpu, LIB_SEED, ids)
    assert tensor.shape == (T, c['B'], c['C'])
    explicit = _run(gpu, name, noise=tensor)
    lib = _run(gpu, name, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids)
    bad = np.argwhere(lib != explicit)
    assert bad.size == 0, f'{name}: {len(bad)} of {lib.size} samples differ from the explicit-tensor run, first at (segment, step) = {tuple(bad[0])}'
    assert len(np.unique(lib)) > 1 and not np.array_equal(lib, c['ref'])        # (another noise stream than the oracle's: another trajectory)
