"""`wrnn_tile_wide_kernel` (csrc/wrnn_tile_wide.hip; algo 'tile' with clusters = W): wrnn_tile_kernel with the rows of every matrix stage spread over W = 2, 4
or 8 workgroups per tile, which hand every stage's output to one another through the workspace.  Its yardstick is exact: an output element is ONE chain of
MFMAs in ascending k on either kernel, so samples and logits must equal `algo='tile'`'s BIT FOR BIT at every width -- and, as that kernel's, stay within the
inherited K * E_ref of the float64 reference and on the C oracle's samples.  Cases, tables, seeds, references and guards are those of tests/test_gpu_tile.py and
tests/test_gpu_fallback_dims.py, imported as they stand:

    T1  RAW  520 / 257  1024 classes  B 17   uneven shares (33 units over 8), an fc stage with 17 units, split RAW logits, a second cluster with ONE live column
    T3  RAW  100 / 50   2 classes     B 33   7 and 4 units and ONE unit of logits: most members idle in every stage; three clusters
    T4  MOL  260 / 33   30            B 18   a row tail, three fc units: members with empty fc shares
    T5  MOL  256 / 256  30            B 32   the aligned case a user brings

Every call is asserted to have run on `wrnn_tile_wide_kernel` (run-info: clusters = W, 16 units per workgroup, one round, one launch)."""
import numpy as np
import pytest
import torch

import test_gpu_tile as tt
from test_gpu_fallback_dims import K, LIB_SEED, T, TF_BAR, _check_samples, _guards
from test_gpu_tile import CASES, TILE, _case, _engine, gpu      # noqa: F401  (gpu: the device fixture)

pytestmark = pytest.mark.gpu

WIDE = 'wrnn_tile_wide_kernel'
WIDTHS = (2, 4, 8)
NAMES = ('T1', 'T3', 'T4', 'T5')
_TILE = {}


def _tile(gpu, name, table='even', forced=False):
    """`algo='tile'` on the same engine, table and noise: computed once, never written to afterwards."""
    key = (name, table, forced)
    if key not in _TILE:
        _TILE[key] = tt._run(gpu, name, table, forced=forced)
    return _TILE[key]


def _wide(gpu, name, W, table='even', forced=False, noise='oracle', segs=None, **kw):
    """`_run` of tests/test_gpu_tile.py with clusters = W, asserting the wide kernel and its run-info."""
    c, eng = _case(name, table), _engine(gpu, name)
    _tile(gpu, name, table)                                       # (puts the case's tensors on the device)
    mels_up, aux, flat, ref = tt._MEMO[('dev', name, table)]
    seg_pos, seg_lim = c['seg_pos'], c['seg_lim']
    if segs is not None:
        seg_pos, seg_lim, B = seg_pos[segs], seg_lim[segs], c['B']
        if c['mode'] == 'MOL':
            flat = torch.cat([flat[:, :10 * B].reshape(T, B, 10)[:, segs].reshape(T, -1), flat[:, 10 * B:][:, segs]], dim=1).contiguous()
        else:
            flat = flat[:, segs].contiguous()
    if forced:
        kw.update(force_x=ref, want_logits=True)
    res = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, flat if noise == 'oracle' else noise, c['hop'], algo='tile', clusters=W, **kw)
    info = eng.last_run_info()
    assert eng.last_loop_kernel() == WIDE and info == dict(kernel=WIDE, units_per_wg=16, clusters=W, depth=0, rounds=1, slab_steps=T, launches=1), info
    return tuple(r.cpu().numpy() for r in res) if forced else res.cpu().numpy()


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert bad.size == 0, f'{what}: {len(bad)} of {a.size} values differ from wrnn_tile_kernel in their bits, first at {tuple(bad[0])}'


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('name', NAMES)
def test_free_run_equals_tile_bit_for_bit(gpu, name, W):
    """The kernel feeds its own samples back -- every member its own copy -- and member 0's `out` is wrnn_tile_kernel's, in both modes."""
    ref = _tile(gpu, name)
    out = _wide(gpu, name, W)
    assert np.array_equal(out, ref)
    _same(out, ref, f'{name} W = {W} samples')
    assert len(np.unique(out)) > 1


@pytest.mark.parametrize('W', WIDTHS)
@pytest.mark.parametrize('name', NAMES)
def test_teacher_forced_logits_and_samples(gpu, name, W):
    """Fed the oracle's samples: the logits are wrnn_tile_kernel's bit for bit (RAW: written by the members that own the rows), within the inherited
    K * E_ref (K = 8, never above TF_BAR) of the float64 reference with the guards in force, and the samples are the oracle's."""
    c = _case(name)
    bound = _guards(c, name)
    t_out, t_logits = _tile(gpu, name, forced=True)
    out, logits = _wide(gpu, name, W, forced=True)
    assert logits.shape == c['lg64'].shape and np.isfinite(logits).all()
    _same(logits, t_logits, f'{name} W = {W} logits')
    _same(out, t_out, f'{name} W = {W} samples')
    err = float(np.abs(logits - c['lg64']).max())
    print(f"{name} W = {W}: E_ref = {c['e_ref']:.3e}, max|hip - float64| = {err:.3e}, err / E_ref = {err / c['e_ref']:.2f}")
    assert err <= bound <= TF_BAR, f"{name} W = {W}: teacher-forced logits off the float64 reference by {err:.3e} = {err / c['e_ref']:.2f} E_ref (bound {K} E_ref)"
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name, W', [('T1', 8), ('T4', 2)])
def test_ragged_segment_table(gpu, name, W):
    """Twelve dead columns beside four live ones, two segments that run out of their utterance mid-way: every member loads the conditioning for itself."""
    c = _case(name, 'ragged')
    _guards(c, name)
    _same(_wide(gpu, name, W, 'ragged'), _tile(gpu, name, 'ragged'), f'{name} ragged samples')
    t_out, t_logits = _tile(gpu, name, 'ragged', forced=True)
    out, logits = _wide(gpu, name, W, 'ragged', forced=True)
    _same(logits, t_logits, f'{name} ragged logits')
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name, W, W2', [('T1', 4, 2), ('T5', 8, 4)])
def test_calls_back_to_back_on_one_workspace(gpu, name, W, W2):
    """Two calls on the SAME workspace, then a third at another width: flags and epochs of a call are its own (the flag block is zeroed in front of every
    launch; a call that found the last epochs of the call before would run ahead of its cluster)."""
    eng, ref = _engine(gpu, name), _tile(gpu, name)
    first = _wide(gpu, name, W)
    ws = eng._ws.data_ptr()
    second = _wide(gpu, name, W)
    assert eng._ws.data_ptr() == ws
    third = _wide(gpu, name, W2)
    assert eng._ws.data_ptr() == ws                               # (the hand-off buffers are sized by tiles and dims, not by the width)
    for out in (first, second, third):
        _same(out, ref, f'{name} samples')


def test_library_noise(gpu):
    """T3 at W = 4: the run that draws its noise inside the call equals the run fed `rng.library_noise`'s tensor, and `algo='tile'` on either."""
    from wavernn_amd.rng import library_noise
    name, W = 'T3', 4
    c = _case(name)
    ids = (np.arange(c['B'], dtype=np.uint64)[::-1] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF0000000000)
    tensor = library_noise(c['mode'], c['B'], 0, T, c['C'], gpu, LIB_SEED, ids)
    explicit = _wide(gpu, name, W, noise=tensor)
    lib = _wide(gpu, name, W, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids)
    _same(lib, explicit, 'library noise')
    _same(lib, tt._run(gpu, name, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids), 'library noise')
    assert len(np.unique(lib)) > 1 and not np.array_equal(lib, c['ref'])


@pytest.mark.parametrize('W', [2, 8])
def test_a_segment_does_not_depend_on_its_tile_mates(gpu, W):
    """tests/test_gpu_tile.py's test, restated under a width: segment 16 of T1 -- alone in the second cluster -- and segment 3 of the first."""
    full = _wide(gpu, 'T1', W)
    lone = _wide(gpu, 'T1', W, segs=slice(16, 17))
    assert lone.shape == (1, T) and np.array_equal(lone[0], full[16]), np.argwhere(lone[0] != full[16])[:4]
    four = _wide(gpu, 'T1', W, segs=slice(0, 4))
    assert four.shape == (4, T) and np.array_equal(four, full[:4])
    assert len(np.unique(full[16])) > 8 and not np.array_equal(full[16], full[3])


@pytest.mark.parametrize('name, W', [('T1', 8), ('T5', 2)])
def test_nll_of_the_wide_calls_logits(gpu, name, W):
    """Scoring: `wrnn_nll` on the wide call's logits gives what it gives on wrnn_tile_kernel's, per step and in sum, bit for bit."""
    from wavernn_amd import _lib
    from wavernn_amd.score import nll_on_device
    c = _case(name)
    target = torch.from_numpy(c['ref']).to(gpu)
    seg_len = torch.full((c['B'],), T, dtype=torch.int32, device=gpu)
    got = []
    for logits in (_tile(gpu, name, forced=True)[1], _wide(gpu, name, W, forced=True)[1]):
        nll, total = nll_on_device(_lib.lib(), 0, c['mode'], torch.from_numpy(logits).to(gpu), target, seg_len, True)
        got.append((nll.cpu().numpy(), total.cpu().numpy()))
    assert np.isfinite(got[0][0]).all() and got[0][1].min() > 0
    _same(got[1][0], got[0][0], 'per-step nll')
    assert np.array_equal(got[1][1], got[0][1])


@pytest.mark.parametrize('W', WIDTHS)
def test_more_segments_than_the_width_takes_are_refused_by_the_planner(gpu, W):
    """ONE round, at most one workgroup per CU: one segment more than (CUs / W) * 16 is the planner's refusal -- in the plan and in the call, which fails
    before anything is queued."""
    from wavernn_amd import _lib
    name = 'T3'
    c, eng = _case(name), _engine(gpu, name)
    most = eng.n_cus // W * 16
    assert eng.plan(most, T, algo='tile', clusters=W)['kernel'] == WIDE
    with pytest.raises(_lib.WrnnError, match=f'at most {most} segments'):
        eng.plan(most + 1, T, algo='tile', clusters=W)
    assert eng.plan(most + 1, T, algo='tile')['kernel'] == TILE
    n = most + 1
    seg_pos, seg_lim = np.resize(c['seg_pos'], n), np.resize(c['seg_lim'], n)
    _tile(gpu, name)
    mels_up, aux, _, _ = tt._MEMO[('dev', name, 'even')]
    noise = torch.ones(T, n, c['C'], device=gpu)
    with pytest.raises(_lib.WrnnError, match=f'at most {most} segments'):
        eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, noise, c['hop'], algo='tile', clusters=W)


def test_model_tile_width(gpu, tmp_path):
    """`model.tile_width = 4` beside `loop_algo = 'tile'` through `generate()`, on the model of tests/test_gpu_tile.py::test_model_loop_algo_tile: the waveform of
    tile_width = 0 bit for bit, and the model names the kernel that ran.  Any other loop_algo refuses the width with its reason."""
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
    model.loop_algo = 'tile'
    outs = {}
    for width, kernel in ((0, TILE), (4, WIDE)):
        model.tile_width = width
        torch.manual_seed(73)
        outs[width] = model.generate(mel, tmp_path / f'w{width}.wav', True, target, overlap, False)
        assert model.last_loop_kernel == kernel, (width, model.last_loop_kernel)
    assert np.array_equal(outs[4], outs[0]) and np.abs(outs[0]).max() > 0.01
    model.loop_algo = 'auto'
    with pytest.raises(ValueError, match="tile_width = 4 needs loop_algo == 'tile'"):
        model.generate(mel, tmp_path / 'refused.wav', True, target, overlap, False)
