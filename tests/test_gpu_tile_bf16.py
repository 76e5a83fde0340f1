"""`wrnn_tile_bf16_kernel` (csrc/wrnn_tile_bf16.hip, algo 'tile_bf16'): wrnn_tile_kernel's dataflow with the eight loop matrices rounded to bfloat16 and every
matrix product on v_mfma_f32_16x16x32_bf16, the float32 activations split into three exact bf16 pieces.  The kernel computes float32 sums of exact
products on the ROUNDED weights, so it is held to what tests/test_gpu_tile.py holds the float32 tile kernel to -- against the references rebuilt on
`bf16_round_state_dict(sd)`, with no loosened tolerance: the cases T1-T5, tables, seeds, K = 8, TF_BAR, `_f64_logits` and `_check_samples` are that file's
and tests/test_gpu_fallback_dims.py's, imported.  The engine under test is built from the UNROUNDED state dict: the rounding is the library's.

The guards, asserted on the CPU before any launch (`_guards_q`): no RAW segment-step of the rounded-weight oracle's run is a near-tie at a relative gap of
1e-4 (100 x the float32 tests' criterion; `_tie`'s computation with that gap); every last-column mutant of the rounded weights moves the float64 logits
by >= 50 K E_ref_q; and so does the rounding itself (max|lg64_q - lg64| >= 50 K E_ref_q), which is what lets test 3 tell rounded weights from float32
ones.  Every case asserts that the call ran on `wrnn_tile_bf16_kernel`."""
import numpy as np
import pytest
import torch

from helpers import MOL_TOL
from test_gpu_fallback_dims import K, LIB_SEED, MATRICES, NSEED, T, TF_BAR, _check_samples, _f64_logits
from test_gpu_tile import CASES, _case as _case_f32

pytestmark = pytest.mark.gpu

BF16, TILE = 'wrnn_tile_bf16_kernel', 'wrnn_tile_kernel'
KERNELS = dict(tile_bf16=BF16, tile=TILE)
TIE_REL_Q = 1e-4
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


# ---- the references (CPU), on the rounded weights ------------------------------------------------------------------------------------------------
def _tie_q(logits, q):
    """`_tie` of tests/test_gpu_fallback_dims.py (float64 p / q on one segment-step) with the relative gap TIE_REL_Q."""
    lg = np.asarray(logits, np.float64)
    p = np.exp(lg - lg.max())
    p /= p.sum()
    r = np.sort(p / np.asarray(q, np.float64))
    return (r[-1] - r[-2]) <= TIE_REL_Q * r[-1]


def _case(name, table='even'):
    """The case of tests/test_gpu_tile.py (weights `sd`, conditioning, table, noise: unchanged) with every reference rebuilt on `sd_q =
    bf16_round_state_dict(sd)`: the C oracle's free run `ref` and float32 logits, `lg64` = the float64 logits teacher-forced with those samples, `e_ref`,
    the near-tie count at 1e-4, what each last-column mutant of the ROUNDED weights moves -- and `lg64_f32`, the float64 logits of the UNROUNDED weights
    under the same fed samples.  Memoised, never written to afterwards."""
    key = (name, table)
    if key in _MEMO:
        return _MEMO[key]
    from oracle import c_oracle as C, wavernn_oracle as O
    from wavernn_amd.synthetic import bf16_round_state_dict
    base = _case_f32(name, table)
    sd, mode, B, hop = base['sd'], base['mode'], base['B'], base['hop']
    sd_q = bf16_round_state_dict(sd)
    M, A = base['cfg']['feat_dims'], base['cfg']['res_out_dims'] // 4
    mels_f, aux_f = np.zeros((B, T, M), np.float32), np.zeros((B, T, 4 * A), np.float32)
    for b in range(B):                              # the gather the kernels do (as `_case` of that file restates it)
        p = int(base['seg_pos'][b]) + np.arange(T)
        ok = p < int(base['seg_lim'][b])
        mels_f[b, ok] = base['mels_up'][p[ok]]
        aux_f[b, ok] = base['aux'][p[ok] // hop]
    noise = O.draw_noise(NSEED, mode, B, T, rnn_dims=base['cfg']['rnn_dims'], aux_dims=A, n_classes=base['C'])
    noise = tuple(np.ascontiguousarray(n, np.float32) for n in noise) if mode == 'MOL' else np.ascontiguousarray(noise, np.float32)
    ref, ref_logits = C.loop(sd_q, mode, mels_f, aux_f, noise, want_logits=True)
    lg64 = _f64_logits(sd_q, mels_f, aux_f, ref)
    e_ref = float(np.abs(ref_logits - lg64).max())
    ties = 0 if mode == 'MOL' else sum(bool(_tie_q(ref_logits[t, b], noise[t, b])) for t in range(T) for b in range(B))
    moved = {}
    for m in MATRICES:
        mutant = dict(sd_q)
        mutant[m] = sd_q[m].copy()
        mutant[m][:, -1] = 0
        moved[m] = float(np.abs(_f64_logits(mutant, mels_f, aux_f, ref) - lg64).max())
    lg64_f32 = _f64_logits(sd, mels_f, aux_f, ref)
    _MEMO[key] = dict(base, sd_q=sd_q, ref=ref, ref_logits=ref_logits, lg64=lg64, e_ref=e_ref, ties=ties, moved=moved, lg64_f32=lg64_f32,
                      rounding_moves=float(np.abs(lg64 - lg64_f32).max()))
    return _MEMO[key]


def _guards_q(c, name):
    bound = K * c['e_ref']
    assert 0 < bound <= TF_BAR, (name, c['e_ref'])
    assert c['ties'] == 0, f"{name}: {c['ties']} segment-steps of the rounded-weight oracle's run are near-ties at {TIE_REL_Q}"
    weak = {m: d for m, d in c['moved'].items() if d < 50 * bound}
    assert not weak, f'{name}: zeroing the last input column moves the float64 logits by less than 50 K E_ref_q = {50 * bound:.2e}: {weak}'
    assert c['rounding_moves'] >= 50 * bound, f"{name}: rounding the weights moves the float64 logits by {c['rounding_moves']:.2e} < 50 K E_ref_q = {50 * bound:.2e}"
    return bound


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------------
def _engine(gpu, name, rounded=False):
    key = ('engine', name, rounded)
    if key not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        c = _case(name)
        _MEMO[key] = LoopEngine(c['sd_q'] if rounded else c['sd'], CASES[name]['mode'], device=gpu)
        assert _MEMO[key].tile_bf16_bytes() > 0
    return _MEMO[key]


def _run(gpu, name, table='even', forced=False, noise='oracle', algo='tile_bf16', segs=None, rounded=False, **kw):
    """One `run_segments` call (as `_run` of tests/test_gpu_tile.py).  forced: fed the rounded-weight oracle's samples, returns (samples, logits)."""
    c, eng = _case(name, table), _engine(gpu, name, rounded)
    key = ('dev', name, table)
    if key not in _MEMO:
        _MEMO[key] = tuple(torch.from_numpy(c[k]).to(gpu) for k in ('mels_up', 'aux', 'flat', 'ref'))
    mels_up, aux, flat, ref = _MEMO[key]
    seg_pos, seg_lim = c['seg_pos'], c['seg_lim']
    if segs is not None:
        assert not forced and noise == 'oracle' and c['mode'] == 'RAW'
        seg_pos, seg_lim, flat = seg_pos[segs], seg_lim[segs], flat[:, segs].contiguous()
    if forced:
        kw.update(force_x=ref, want_logits=True)
    res = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, flat if noise == 'oracle' else noise, c['hop'], algo=algo, **kw)
    assert eng.last_loop_kernel() == KERNELS[algo], (name, algo, eng.last_loop_kernel())
    return tuple(r.cpu().numpy() for r in res) if forced else res.cpu().numpy()


def _forced(gpu, name, table='even', **kw):
    key = ('forced', name, table, tuple(sorted(kw.items())))
    if key not in _MEMO:
        _MEMO[key] = _run(gpu, name, table, forced=True, **kw)
    return _MEMO[key]


def _check_forced(gpu, name, table):
    c = _case(name, table)
    bound = _guards_q(c, name)
    out, logits = _forced(gpu, name, table)
    assert logits.shape == c['lg64'].shape and np.isfinite(logits).all()
    err = float(np.abs(logits - c['lg64']).max())
    print(f"{name} {table}: E_ref_q = {c['e_ref']:.3e}, max|hip - float64 (rounded weights)| = {err:.3e}, err / E_ref_q = {err / c['e_ref']:.2f}, "
          f"weakest mutant moves {min(c['moved'].values()):.2e}, the rounding moves {c['rounding_moves']:.2e}")
    assert err <= bound <= TF_BAR, \
        f"{name} {table}: teacher-forced logits off the float64 reference on the rounded weights by {err:.3e} = {err / c['e_ref']:.2f} E_ref_q (bound {K} E_ref_q)"
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name,table', [(n, 'even') for n in CASES] + [('T1', 'ragged'), ('T4', 'ragged')])
def test_teacher_forced_logits_and_samples(gpu, name, table):
    """1. Fed the rounded-weight oracle's samples, every step's logits stay within K * E_ref_q of the float64 reference ON THE ROUNDED WEIGHTS, and the
    samples drawn from them are that oracle's (RAW: the same class index at every (segment, step); MoL: within MOL_TOL).

    Measured on an MI355X with K = 8 in force (err = max|hip - float64 on the rounded weights|; the largest ratio is 0.98, below 4, so K stays 8 -- the
    bf16 MFMA's internal adder keeps the kernel where the float32 tile kernel is, 0.93 ... 1.21):
        case        E_ref_q    err        err / E_ref_q   weakest mutant moves   the rounding moves
        T1          1.85e-07   1.29e-07   0.70            1.78e-03               6.90e-04
        T2          2.69e-07   1.70e-07   0.63            4.33e-03               1.02e-03
        T3          4.51e-08   4.08e-08   0.91            1.18e-03               3.70e-04
        T4          2.13e-07   2.08e-07   0.98            1.68e-03               9.33e-04
        T5          2.32e-07   1.98e-07   0.86            1.94e-03               7.09e-04
        T1 ragged   1.76e-07   1.19e-07   0.68            1.60e-03               6.46e-04
        T4 ragged   1.78e-07   1.58e-07   0.89            1.51e-03               8.98e-04
    (needed of the last two columns: 50 K E_ref_q <= 1.07e-04.)"""
    _check_forced(gpu, name, table)


@pytest.mark.parametrize('name', list(CASES))
def test_free_run(gpu, name):
    """2. No force_x: the kernel feeds its own samples back and walks the rounded-weight oracle's trajectory."""
    c = _case(name)
    _guards_q(c, name)
    _check_samples(c, name, _run(gpu, name), 'free run')


@pytest.mark.parametrize('name', list(CASES))
def test_the_weights_are_rounded_to_nearest(gpu, name):
    """3. The teacher-forced logits of test 1 are FARTHER than 50 K E_ref_q from the float64 logits of the unrounded weights under the same fed samples: a
    kernel that read float32 weights would sit within K E_ref of those (and one that truncated instead of rounding fails test 1)."""
    c = _case(name)
    bound = _guards_q(c, name)
    _, logits = _forced(gpu, name)
    off = float(np.abs(logits - c['lg64_f32']).max())
    print(f"{name}: max|hip - float64 (unrounded weights)| = {off:.3e}, 50 K E_ref_q = {50 * bound:.3e}")
    assert off > 50 * bound


@pytest.mark.parametrize('name', list(CASES))
def test_rounding_is_idempotent(gpu, name):
    """4. An engine built from the already rounded state dict gives bit-identical samples and logits under 'tile_bf16'; under 'tile' -- the float32 MFMA on
    the rounded weights -- its logits are within 2 K E_ref_q of tile_bf16's and RAW samples are equal (MoL: within MOL_TOL)."""
    c = _case(name)
    bound = _guards_q(c, name)
    out, logits = _forced(gpu, name)
    out_q, logits_q = _run(gpu, name, forced=True, rounded=True)
    assert np.array_equal(out_q.view(np.uint32), out.view(np.uint32)) and np.array_equal(logits_q.view(np.uint32), logits.view(np.uint32))
    out_t, logits_t = _run(gpu, name, forced=True, rounded=True, algo='tile')
    err = float(np.abs(logits_t - logits).max())
    print(f"{name}: max|tile on the rounded weights - tile_bf16| = {err:.3e} = {err / c['e_ref']:.2f} E_ref_q")
    assert err <= 2 * bound
    if c['mode'] == 'RAW':
        assert np.array_equal(out_t, out)
    else:
        assert float(np.abs(out_t - out).max()) <= MOL_TOL


def test_a_segment_does_not_depend_on_its_tile_mates(gpu):
    """5. T1: segment 16 alone and segments 0-3 alone are bit-identical to the 17-segment run, as in tests/test_gpu_tile.py."""
    full = _run(gpu, 'T1')
    lone = _run(gpu, 'T1', segs=slice(16, 17))
    assert lone.shape == (1, T) and np.array_equal(lone[0], full[16]), np.argwhere(lone[0] != full[16])[:4]
    four = _run(gpu, 'T1', segs=slice(0, 4))
    assert four.shape == (4, T) and np.array_equal(four[3], full[3]) and np.array_equal(four, full[:4])
    assert len(np.unique(full[16])) > 8 and not np.array_equal(full[16], full[3])


def test_library_noise(gpu):
    """6. T3: the run that draws its noise inside the call equals, sample for sample, the run fed `rng.library_noise`'s tensor."""
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
    assert len(np.unique(lib)) > 1 and not np.array_equal(lib, c['ref'])


def _model_256(gpu, rounded):
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import bf16_round_state_dict, random_state_dict
    hp = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
              hop_length=128, sample_rate=16000)
    sd = random_state_dict(71, mode='MOL', **hp)
    if rounded:
        sd = bf16_round_state_dict(sd)
    model = WaveRNN(**hp, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return model.to(gpu), sd, hp


def test_model_loop_algo_tile_bf16(gpu, tmp_path):
    """7. `model.loop_algo = 'tile_bf16'` through `generate()`: the 256 / 256 MoL model and the 30-frame mel of test_model_loop_algo_tile give the waveform of
    `loop_algo = 'tile'` on a model loaded with the ROUNDED weights to MOL_TOL, and the model names the kernel that ran."""
    from wavernn_amd import fold
    from wavernn_amd.synthetic import random_mel
    mel = torch.tensor(random_mel(72, 30, n_mels=80)).unsqueeze(0)
    target, overlap = 200, 16
    assert fold.fold_geometry(30 * 128, target, overlap)[0] >= 17
    outs = {}
    for algo, rounded in (('tile_bf16', False), ('tile', True)):
        model = _model_256(gpu, rounded)[0]
        model.loop_algo = algo
        torch.manual_seed(73)
        outs[algo] = model.generate(mel, tmp_path / f'{algo}.wav', True, target, overlap, False)
        assert model.last_loop_kernel == KERNELS[algo], (algo, model.last_loop_kernel)
    assert outs['tile_bf16'].shape == outs['tile'].shape and np.isfinite(outs['tile_bf16']).all()
    err = float(np.abs(outs['tile_bf16'] - outs['tile']).max())
    assert err <= MOL_TOL, f'max|tile_bf16 - tile on the rounded weights| = {err:.3e}'
    assert np.abs(outs['tile']).max() > 0.01


def test_scoring(gpu):
    """8. The 256 / 256 model of test_other_model_dims_score_on_the_fallback_kernels under `score_corpus(..., algo='tile_bf16')`: per-step values within
    bound_of('MOL') of `nll_host` on the oracle's teacher-forced logits ON THE ROUNDED WEIGHTS."""
    from oracle import wavernn_oracle as O
    from test_gpu_score import bound_of, oracle_forced_logits, short_wave
    from wavernn_amd import _lib
    from wavernn_amd.batch import score_corpus
    from wavernn_amd.score import prepare_targets
    from wavernn_amd.synthetic import bf16_round_state_dict, random_mel
    model, sd, hp = _model_256(gpu, False)
    sd_q = bf16_round_state_dict(sd)
    mel, steps = random_mel(72, 3), 3 * 128
    wav = short_wave(steps, 11)
    m = O.pad_tensor(mel.T[None], 2, 'both')[0].T
    mels_up, aux_up = O.upsample_network(sd_q, m, hp['upsample_factors'], 2)
    x = prepare_targets(wav, 'MOL')[1]
    ref = _lib.nll_host('MOL', oracle_forced_logits(sd_q, mels_up[None], aux_up[None], x), x[None])[0][0]
    bound = bound_of('MOL')
    r = score_corpus(model, [torch.from_numpy(mel).unsqueeze(0)] * 2, [wav, wav[:200]], per_step=True, algo='tile_bf16')
    assert model.last_loop_kernel == BF16, model.last_loop_kernel
    err = max(float(np.abs(r[0]['per_step'] - ref).max()), float(np.abs(r[1]['per_step'] - ref[:200]).max()))
    print(f'{BF16}: max per-step |ours - oracle on the rounded weights| = {err:.3e} (bound {bound:.3e})')
    assert r[0]['steps'] == steps and r[1]['steps'] == 200 and err <= bound


def test_a_pack_whose_weight_rounds_to_inf_has_no_view_and_is_refused(gpu):
    """A weight above the largest bfloat16 (T3's fc3, one value of 3.4e38): `wrnn_pack_create` succeeds without the view, `tile_bf16` is refused with a
    text that says why, and `tile` still plans the pack."""
    from wavernn_amd import _lib
    from wavernn_amd.engine import LoopEngine
    sd = dict(_case('T3')['sd'])
    sd['fc3.weight'] = sd['fc3.weight'].copy()
    sd['fc3.weight'][1, 7] = np.float32(3.4e38)
    eng = LoopEngine(sd, 'RAW', device=gpu)
    assert eng.tile_bf16_bytes() == 0 and _engine(gpu, 'T3').tile_bf16_bytes() > 0
    with pytest.raises(_lib.WrnnError, match='no bf16 view'):
        eng.plan(33, T, algo='tile_bf16')
    eng.plan(33, T, algo='tile')
