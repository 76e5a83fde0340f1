"""`wrnn_tile_kernel` (csrc/wrnn_tile.hip, algo 'tile'): wrnn_generic_kernel's dataflow for a tile of up to 16 segments per workgroup, every matrix product
on v_mfma_f32_16x16x4_f32.  The method is that of tests/test_gpu_fallback_dims.py, taken over as it stands (its helpers are imported; its cases are its own):
the C oracle's free run, `_f64_logits` teacher-forced with the oracle's samples, the logits bound K * E_ref (K = 8, never above TF_BAR = 1e-4), and the
`_guards` on the inputs -- no RAW near-tie at relative 1e-6, and every last-column mutant moves the float64 logits by >= 50 K E_ref -- so nothing is excused
and RAW class indices are demanded EQUAL.  Every case asserts that the call ran on `wrnn_tile_kernel`.

    id  mode  rnn   fc   classes  feat  res_out  B   what it reaches
    T1  RAW   520   257  1024     13    20       17  a row tail (520 = 32 tiles + 8 rows), an odd F, K tails (K0 = 19, H + A = 525), a second workgroup with ONE
                                                     live column
    T2  RAW   72    600  1024     80    128      16  F > H, exactly one full tile, the 16-segment RAW sampler over 1024 classes
    T3  RAW   100   50   2        7     4        33  a class tile with 2 live rows, A = 1, three workgroups of which the last has one live column
    T4  MOL   260   33   30       3     12       18  a K tail of 0 with a row tail of 4, F below a tile multiple, MoL sampling in a 2-column tile
    T5  MOL   256   256  30       80    128      32  what a user is most likely to bring: everything aligned, two full tiles

The even table (hop 8, stride 21), the 4-segment 'ragged' table and the seeds (weights 5, mel / aux 1, noise 7) are that file's."""
import numpy as np
import pytest
import torch

from helpers import MOL_TOL
from test_gpu_fallback_dims import (HOP, K, LIB_SEED, MATRICES, MSEED, NSEED, RAGGED_HOP, STRIDE, T, TF_BAR, WSEED, _check_samples, _f64_logits, _guards,
                                    _tie)

pytestmark = pytest.mark.gpu

TILE, GENERIC = 'wrnn_tile_kernel', 'wrnn_generic_kernel'
CASES = {
    'T1': dict(mode='RAW', rnn_dims=520, fc_dims=257, bits=10, feat_dims=13, res_out_dims=20, B=17),
    'T2': dict(mode='RAW', rnn_dims=72, fc_dims=600, bits=10, feat_dims=80, res_out_dims=128, B=16),
    'T3': dict(mode='RAW', rnn_dims=100, fc_dims=50, bits=1, feat_dims=7, res_out_dims=4, B=33),
    'T4': dict(mode='MOL', rnn_dims=260, fc_dims=33, bits=9, feat_dims=3, res_out_dims=12, B=18),
    'T5': dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128, B=32),
}
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


# ---- the references (CPU): `_table` and `_case` of tests/test_gpu_fallback_dims.py, restated over the cases of this file ------------------------
def _table(name, table):
    if table == 'ragged':
        return RAGGED_HOP, np.array([0, 45, 91, 141], np.int32), np.array([91, 91, 196, 196], np.int32), 196
    B = CASES[name]['B']
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    return HOP, np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32), L


def _case(name, table='even'):
    """Everything the CPU knows about a case (memoised, never written to afterwards): weights, conditioning, segment table, noise, the C oracle's free run,
    the float64 logits teacher-forced with its samples, E_ref, the near-tie count and what each last-column mutant moves."""
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


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------------
def _engine(gpu, name):
    if ('engine', name) not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        _MEMO[('engine', name)] = LoopEngine(_case(name)['sd'], CASES[name]['mode'], device=gpu)
    return _MEMO[('engine', name)]


def _run(gpu, name, table='even', forced=False, noise='oracle', algo='tile', segs=None, **kw):
    """One `run_segments` call of a case on its table.  forced: fed the oracle's samples, returns (samples, logits), else the samples.  segs: a slice of the
    table's segments run ALONE, with their own rows of the table and of the oracle's noise."""
    c, eng = _case(name, table), _engine(gpu, name)
    key = ('dev', name, table)
    if key not in _MEMO:
        _MEMO[key] = tuple(torch.from_numpy(c[k]).to(gpu) for k in ('mels_up', 'aux', 'flat', 'ref'))
    mels_up, aux, flat, ref = _MEMO[key]
    seg_pos, seg_lim = c['seg_pos'], c['seg_lim']
    if segs is not None:
        assert not forced and noise == 'oracle'
        seg_pos, seg_lim, B = seg_pos[segs], seg_lim[segs], c['B']
        if c['mode'] == 'MOL':      # [T][10 B | B]
            flat = torch.cat([flat[:, :10 * B].reshape(T, B, 10)[:, segs].reshape(T, -1), flat[:, 10 * B:][:, segs]], dim=1).contiguous()
        else:                       # [T][B][C]
            flat = flat[:, segs].contiguous()
    if forced:
        kw.update(force_x=ref, want_logits=True)
    res = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, flat if noise == 'oracle' else noise, c['hop'], algo=algo, **kw)
    assert eng.last_loop_kernel() == (TILE if algo == 'tile' else GENERIC), (name, algo, eng.last_loop_kernel())
    return tuple(r.cpu().numpy() for r in res) if forced else res.cpu().numpy()


def _check_forced(gpu, name, table):
    c = _case(name, table)
    bound = _guards(c, name)
    out, logits = _run(gpu, name, table, forced=True)
    assert logits.shape == c['lg64'].shape and np.isfinite(logits).all()
    err = float(np.abs(logits - c['lg64']).max())
    print(f"{name} {table}: E_ref = {c['e_ref']:.3e}, max|hip - float64| = {err:.3e}, err / E_ref = {err / c['e_ref']:.2f}, "
          f"weakest mutant moves {min(c['moved'].values()):.2e}")
    assert err <= bound <= TF_BAR, f"{name} {table}: teacher-forced logits off the float64 reference by {err:.3e} = {err / c['e_ref']:.2f} E_ref (bound {K} E_ref)"
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name', list(CASES))
def test_teacher_forced_logits_and_samples(gpu, name):
    """Fed the oracle's samples, every step's logits stay within K * E_ref of the float64 reference, and the samples drawn from them are the oracle's
    (RAW: the same class index at every (segment, step); MoL: within MOL_TOL).

    Measured on an MI355X with K = 8 in force (err = max|hip - float64|; no ratio is above 1.21, so K stays 8):
        case        E_ref      err        err / E_ref   weakest mutant moves
        T1          1.65e-07   1.66e-07   1.01          1.79e-03
        T2          2.08e-07   2.10e-07   1.01          4.32e-03
        T3          3.92e-08   4.34e-08   1.10          1.17e-03
        T4          2.00e-07   2.10e-07   1.05          1.68e-03
        T5          2.24e-07   2.20e-07   0.98          1.96e-03
        T1 ragged   1.47e-07   1.77e-07   1.21          1.60e-03
        T4 ragged   1.90e-07   1.76e-07   0.93          1.51e-03"""
    _check_forced(gpu, name, 'even')


@pytest.mark.parametrize('name', list(CASES))
def test_free_run(gpu, name):
    """No force_x: the kernel feeds its own samples back and must walk the oracle's trajectory."""
    c = _case(name)
    _guards(c, name)
    _check_samples(c, name, _run(gpu, name), 'free run')


@pytest.mark.parametrize('name', ['T1', 'T4'])
def test_ragged_segment_table(gpu, name):
    """The kernel's own segment-table handling (`live = p < lim`, zeros past an utterance, aux row p / hop) on the 4-segment 'ragged' table: two utterances
    end to end, hop 7, two segments that run out of their utterance mid-way -- twelve dead columns beside four live ones."""
    _check_forced(gpu, name, 'ragged')
    _check_samples(_case(name, 'ragged'), name, _run(gpu, name, 'ragged'), 'free run')


def test_a_segment_does_not_depend_on_its_tile_mates(gpu):
    """T1: the samples of segment 16 -- alone in the second workgroup of the 17-segment run -- and of segment 3 of the first tile are bit-identical to those
    of a run without the others (segment 16 alone; segments 0-3 alone), given the same table rows and noise rows: a wave runs the whole K of an output
    element itself, so its summation order depends on neither the wave count nor the tile's other columns."""
    full = _run(gpu, 'T1')
    lone = _run(gpu, 'T1', segs=slice(16, 17))
    assert lone.shape == (1, T) and np.array_equal(lone[0], full[16]), np.argwhere(lone[0] != full[16])[:4]
    four = _run(gpu, 'T1', segs=slice(0, 4))
    assert four.shape == (4, T) and np.array_equal(four[3], full[3]) and np.array_equal(four, full[:4])
    assert len(np.unique(full[16])) > 8 and not np.array_equal(full[16], full[3])


@pytest.mark.parametrize('name', ['T2', 'T4'])
def test_against_the_generic_kernel(gpu, name):
    """The same call under algo='auto' runs wrnn_generic_kernel (one fmaf chain per dot product): RAW samples are equal, MoL within MOL_TOL."""
    c = _case(name)
    _guards(c, name)
    tile, generic = _run(gpu, name), _run(gpu, name, algo='auto')
    if c['mode'] == 'MOL':
        err = float(np.abs(tile - generic).max())
        assert err <= MOL_TOL, f'{name}: max|tile - generic| = {err:.3e}'
    else:
        bad = np.argwhere(tile != generic)
        assert bad.size == 0, f'{name}: {len(bad)} of {tile.size} samples differ from the generic kernel, first at (segment, step) = {tuple(bad[0])}'


def test_library_noise(gpu):
    """T3: the run that draws its noise inside the call (`noise=None` + `noise_seed`, a reversed, scrambled id list) equals, sample for sample, the run fed
    `rng.library_noise`'s tensor."""
    from wavernn_amd.rng import library_noise
    name = 'T3'
    c = _case(name)
    ids = (np.arange(c['B'], dtype=np.uint64)[::-1] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF0000000000)
    tensor = library_noise(c['mode'], c['B'], 0, T, c['C'], gpu, LIB_SEED, ids)
    assert tensor.shape == (T, c['B'], c['C'])
    explicit = _run(gpu, name, noise=tensor)
    lib = _run(gpu, name, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids)
    bad = np.argwhere(lib != explicit)
    assert bad.size == 0, f'{name}: {len(bad)} of {lib.size} samples differ from the explicit-tensor run, first at (segment, step) = {tuple(bad[0])}'
    assert len(np.unique(lib)) > 1 and not np.array_equal(lib, c['ref'])        # (another noise stream than the oracle's: another trajectory)


def test_model_loop_algo_tile(gpu, tmp_path):
    """`model.loop_algo = 'tile'` through `generate()`: a MoL model of T5's dims, batched, a 30-frame mel folded into >= 17 segments (two workgroups) gives
    the waveform of `loop_algo = 'auto'` (wrnn_generic_kernel) to MOL_TOL, and the model names the kernel that ran."""
    from wavernn_amd import fold
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, random_mel
    hp = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
              hop_length=128, sample_rate=16000)
    sd = random_state_dict(71, mode='MOL', **hp)
    model = WaveRNN(**hp, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(gpu)
    mel = torch.tensor(random_mel(72, 30, n_mels=80)).unsqueeze(0)
    target, overlap = 200, 16
    assert fold.fold_geometry(30 * 128, target, overlap)[0] >= 17
    outs = {}
    for algo, kernel in (('tile', TILE), ('auto', GENERIC)):
        model.loop_algo = algo
        torch.manual_seed(73)
        outs[algo] = model.generate(mel, tmp_path / f'{algo}.wav', True, target, overlap, False)
        assert model.last_loop_kernel == kernel, (algo, model.last_loop_kernel)
    assert outs['tile'].shape == outs['auto'].shape and np.isfinite(outs['tile']).all()
    err = float(np.abs(outs['tile'] - outs['auto']).max())
    assert err <= MOL_TOL, f'max|tile - auto| = {err:.3e}'
    assert np.abs(outs['auto']).max() > 0.01
