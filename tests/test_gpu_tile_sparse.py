"""`wrnn_tile_sparse_kernel` (csrc/wrnn_tile_sparse.hip, algo 'tile_sparse'): wrnn_tile_kernel's dataflow with the GRU matrices -- and fc1 / fc2 -- of a
pruned model of non-shipped dims run as gathered block-sparse MFMA stages over the pack's tile-sparse view.  The method is that of
tests/test_gpu_fallback_dims.py / tests/test_gpu_tile.py (helpers imported): the C oracle's free run on the MASKED DENSE weights, `_f64_logits`
teacher-forced with the oracle's samples, the logits bound K * E_ref (K = 8, never above TF_BAR = 1e-4), RAW class indices EQUAL, MoL samples within MOL_TOL.
Every case asserts that the call ran on `wrnn_tile_sparse_kernel`.  T = 64, the even table (hop 8, stride 21); seeds: weights 5, mel / aux 1, noise 7;
weights `random_state_dict(5, compute_dims=8, res_blocks=1, ...)`, then `block_prune_state_dict`.

    id   mode  rnn  fc   classes  feat  res_out  B   pruned    sparsity  what it reaches
    P1   MOL   256  256  30       80    128      18  GRU + fc  0.90      aligned dims; a second workgroup with 2 live columns; 14-40 columns per block row
    P2   RAW   144  80   1024     13    20       17  GRU + fc  0.75      9 block rows per gate: a wave's share has a tail; K = 149 and 85: aux columns in the
                                                                         lists, K no multiple of 4; lists of 15-49
    P3   MOL   320  48   30       3     12       33  GRU only  0.95      dense fc stages beside sparse GRU stages; lists of 5-26; three workgroups, the last
                                                                         with one live column
    P3e  as P3, then in rnn1.weight_hh_l0: block row 0 of every gate zeroed, block row 1 of gate 0 restored from the unpruned matrix; B = 16: empty lists
         and a full one (320 columns)

The guards (`_guards`, asserted before anything is launched): the bound is <= 1e-4, no RAW segment-step is a near-tie, and the mutants -- the last-column
mutants restated for lists: for each pruned matrix the LAST surviving block of every block row zeroed, and separately the FIRST, the terms a wrong list
length, offset or padding rule would drop -- each move the float64 logits by >= 50 K E_ref."""
import numpy as np
import pytest
import torch

from helpers import MOL_TOL
from test_gpu_fallback_dims import HOP, K, LIB_SEED, MSEED, NSEED, RAGGED_HOP, STRIDE, T, TF_BAR, WSEED, _check_samples, _f64_logits, _guards, _tie

pytestmark = pytest.mark.gpu

SPARSE, TILE = 'wrnn_tile_sparse_kernel', 'wrnn_tile_kernel'
GRU = ('rnn1.weight_ih_l0', 'rnn1.weight_hh_l0', 'rnn2.weight_ih_l0', 'rnn2.weight_hh_l0')
FC = ('fc1.weight', 'fc2.weight')
CASES = {
    'P1': dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128, B=18, sparsity=0.90, linear=True),
    'P2': dict(mode='RAW', rnn_dims=144, fc_dims=80, bits=10, feat_dims=13, res_out_dims=20, B=17, sparsity=0.75, linear=True),
    'P3': dict(mode='MOL', rnn_dims=320, fc_dims=48, bits=9, feat_dims=3, res_out_dims=12, B=33, sparsity=0.95, linear=False),
    'P3e': dict(mode='MOL', rnn_dims=320, fc_dims=48, bits=9, feat_dims=3, res_out_dims=12, B=16, sparsity=0.95, linear=False, edit=True),
}
HP = ('mode', 'rnn_dims', 'fc_dims', 'bits', 'feat_dims', 'res_out_dims')
_MEMO = {}


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


# ---- the references (CPU) ------------------------------------------------------------------------------------------------------------------------
def _weights(name, pruned=True):
    """The (pruned) state dict of a case; memoised, never written to."""
    key = ('sd', name, pruned)
    if key not in _MEMO:
        from wavernn_amd.prune import block_prune_state_dict
        from wavernn_amd.synthetic import random_state_dict
        cfg = CASES[name]
        dense = random_state_dict(WSEED, compute_dims=8, res_blocks=1, **{k: cfg[k] for k in HP})
        sd, _ = block_prune_state_dict(dense, cfg['sparsity'], linear=cfg['linear'])
        if cfg.get('edit'):
            H = cfg['rnn_dims']
            W = sd['rnn1.weight_hh_l0'].copy()
            for g in range(3):
                W[g * H:g * H + 16] = 0
            W[16:32] = dense['rnn1.weight_hh_l0'][16:32]
            assert np.count_nonzero(np.abs(W[16:32]).max(axis=0)) == H         # a full list
            sd['rnn1.weight_hh_l0'] = W
        _MEMO[('sd', name, True)], _MEMO[('sd', name, False)] = sd, dense
    return _MEMO[key]


def _list_mutants(sd, name):
    """{label: state dict}: per pruned matrix, the last -- and separately the first -- surviving block of every block row zeroed."""
    out = {}
    for m in GRU + (FC if CASES[name]['linear'] else ()):
        for which in ('last', 'first'):
            W = sd[m].copy()
            for br in range(W.shape[0] // 16):
                cols = np.flatnonzero(np.abs(W[16 * br:16 * br + 16]).max(axis=0))
                if len(cols):
                    W[16 * br:16 * br + 16, cols[-1 if which == 'last' else 0]] = 0
            mutant = dict(sd)
            mutant[m] = W
            out[f'{m} {which}'] = mutant
    return out


def _table(name, table):
    if table == 'ragged':
        return RAGGED_HOP, np.array([0, 45, 91, 141], np.int32), np.array([91, 91, 196, 196], np.int32), 196
    B = CASES[name]['B']
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    return HOP, np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32), L


def _case(name, table='even'):
    """Everything the CPU knows about a case (memoised, never written to afterwards): `_case` of tests/test_gpu_fallback_dims.py on the pruned weights,
    with the list mutants in the place of the last-column mutants."""
    key = (name, table)
    if key in _MEMO:
        return _MEMO[key]
    from oracle import c_oracle as C, wavernn_oracle as O
    cfg, sd = CASES[name], _weights(name)
    mode, H, M, A = cfg['mode'], cfg['rnn_dims'], cfg['feat_dims'], cfg['res_out_dims'] // 4
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
    moved = {label: float(np.abs(_f64_logits(mutant, mels_f, aux_f, ref) - lg64).max()) for label, mutant in _list_mutants(sd, name).items()}
    _MEMO[key] = dict(cfg=cfg, sd=sd, mode=mode, C=n_classes, B=B, hop=hop, seg_pos=seg_pos, seg_lim=seg_lim, mels_up=mels_up, aux=aux, flat=flat,
                      ref=ref, ref_logits=ref_logits, lg64=lg64, e_ref=e_ref, ties=ties, moved=moved)
    return _MEMO[key]


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------------
def _engine(gpu, name):
    if ('engine', name) not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        eng = LoopEngine(_weights(name), CASES[name]['mode'], device=gpu)
        view, kept, total = eng.tile_sparse_view()
        assert view == (2 if CASES[name]['linear'] else 1), (name, view, kept, total)
        assert all(100 * k <= 41 * t for k, t in zip(kept[:4], total[:4])) and eng.sparse_blocks == -CASES[name]['rnn_dims'] and eng.sparse_fc_blocks == 0
        _MEMO[('engine', name)] = eng
    return _MEMO[('engine', name)]


def _run(gpu, name, table='even', forced=False, noise='oracle', algo='tile_sparse', segs=None, **kw):
    """One `run_segments` call of a case on its table (`_run` of tests/test_gpu_tile.py).  forced: fed the oracle's samples, returns (samples, logits), else
    the samples.  segs: a list of the table's segments run ALONE, with their own rows of the table and of the oracle's noise."""
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
    assert eng.last_loop_kernel() == (SPARSE if algo == 'tile_sparse' else TILE), (name, algo, eng.last_loop_kernel())
    return tuple(r.cpu().numpy() for r in res) if forced else res.cpu().numpy()


def _check_forced(gpu, name, table):
    c = _case(name, table)
    bound = _guards(c, name)
    out, logits = _run(gpu, name, table, forced=True)
    assert logits.shape == c['lg64'].shape and np.isfinite(logits).all()
    err = float(np.abs(logits - c['lg64']).max())
    # the observation (recorded, not asserted): are the logits those of wrnn_tile_kernel on the masked weights, bit for bit?
    _, dense = _run(gpu, name, table, forced=True, algo='tile')
    same = np.array_equal(logits.view(np.uint32), dense.view(np.uint32))
    print(f"{name} {table}: E_ref = {c['e_ref']:.3e}, max|hip - float64| = {err:.3e}, err / E_ref = {err / c['e_ref']:.2f}, "
          f"weakest mutant moves {min(c['moved'].values()):.2e} (needed {50 * bound:.2e}); logits bit-identical to wrnn_tile_kernel's: {same}, "
          f"max|tile_sparse - tile| = {float(np.abs(logits - dense).max()):.3e}")
    assert err <= bound <= TF_BAR, f"{name} {table}: teacher-forced logits off the float64 reference by {err:.3e} = {err / c['e_ref']:.2f} E_ref (bound {K} E_ref)"
    _check_samples(c, name, out, 'teacher-forced')


@pytest.mark.parametrize('name', list(CASES))
def test_teacher_forced_logits_and_samples(gpu, name):
    """Fed the oracle's samples, every step's logits stay within K * E_ref of the float64 reference, and the samples drawn from them are the oracle's
    (RAW: the same class index at every (segment, step); MoL: within MOL_TOL)."""
    _check_forced(gpu, name, 'even')


@pytest.mark.parametrize('name', list(CASES))
def test_free_run(gpu, name):
    """No force_x: the kernel feeds its own samples back and must walk the oracle's trajectory."""
    c = _case(name)
    _guards(c, name)
    _check_samples(c, name, _run(gpu, name), 'free run')


def test_ragged_segment_table(gpu):
    """P2 on the 4-segment 'ragged' table of tests/test_gpu_fallback_dims.py: two utterances end to end, hop 7, two segments that run out of their utterance
    mid-way -- twelve dead columns beside four live ones."""
    _check_forced(gpu, 'P2', 'ragged')
    _check_samples(_case('P2', 'ragged'), 'P2', _run(gpu, 'P2', 'ragged'), 'free run')


@pytest.mark.parametrize('name', ['P1', 'P2'])
def test_library_noise(gpu, name):
    """The run that draws its noise inside the call (`noise=None` + `noise_seed`, a reversed, scrambled id list) gives what the same call gives on
    wrnn_tile_kernel, which runs the masked weights dense: RAW sample for sample, MoL within MOL_TOL."""
    c = _case(name)
    ids = (np.arange(c['B'], dtype=np.uint64)[::-1] * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0xABCDEF0000000000)
    sparse = _run(gpu, name, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids)
    dense = _run(gpu, name, noise=None, noise_seed=LIB_SEED, noise_seg_id=ids, algo='tile')
    if c['mode'] == 'MOL':
        err = float(np.abs(sparse - dense).max())
        assert err <= MOL_TOL, f'{name}: max|tile_sparse - tile| = {err:.3e}'
    else:
        bad = np.argwhere(sparse != dense)
        assert bad.size == 0, f'{name}: {len(bad)} of {sparse.size} samples differ from wrnn_tile_kernel, first at (segment, step) = {tuple(bad[0])}'
    assert len(np.unique(sparse)) > 1 and not np.array_equal(sparse, c['ref'])        # (another noise stream than the oracle's: another trajectory)


def test_a_segment_does_not_depend_on_its_tile_mates(gpu):
    """P1: segments 0, 16 and 17 -- the first of the first workgroup and the two live columns of the second -- run alone, as one 3-column tile, give the bits
    they give inside the 18-segment run: an output element is one chain over its block row's list, whatever rides along."""
    full = _run(gpu, 'P1')
    lone = _run(gpu, 'P1', segs=[0, 16, 17])
    assert lone.shape == (3, T) and np.array_equal(lone.view(np.uint32), full[[0, 16, 17]].view(np.uint32)), np.argwhere(lone != full[[0, 16, 17]])[:4]
    assert len(np.unique(full[16])) > 8 and not np.array_equal(full[16], full[0])


def test_against_the_dense_tile_kernel(gpu):
    """P2: the RAW class indices of `tile_sparse` are those of `tile` on the same pack."""
    _guards(_case('P2'), 'P2')
    sparse, dense = _run(gpu, 'P2'), _run(gpu, 'P2', algo='tile')
    bad = np.argwhere(sparse != dense)
    assert bad.size == 0, f'P2: {len(bad)} of {sparse.size} samples differ from wrnn_tile_kernel, first at (segment, step) = {tuple(bad[0])}'


def test_a_dense_generic_pack_is_refused_with_the_planners_text(gpu):
    from wavernn_amd import _lib
    from wavernn_amd.engine import LoopEngine
    c = _case('P1')
    eng = LoopEngine(_weights('P1', pruned=False), 'MOL', device=gpu)
    view, kept, total = eng.tile_sparse_view()
    assert view == 0 and kept[:4] == total[:4] and total[0] == 3 * 16 * 256 and total[2] == 3 * 16 * 288
    mels_up, aux, flat = (torch.from_numpy(c[k]).to(gpu) for k in ('mels_up', 'aux', 'flat'))
    with pytest.raises(_lib.WrnnError, match=r'wrnn_tile_sparse_kernel: this pack has no tile-sparse view -- 100\.0 % of the 16x1 blocks of rnn1\.weight_ih survive'):
        eng.run_segments(mels_up, aux, c['seg_pos'], c['seg_lim'], T, flat, c['hop'], algo='tile_sparse')
    out = eng.run_segments(mels_up, aux, c['seg_pos'], c['seg_lim'], T, flat, c['hop'], algo='tile')        # `tile` runs it, as before
    assert eng.last_loop_kernel() == TILE and np.isfinite(out.cpu().numpy()).all()


def test_a_pack_of_the_shipped_dims_is_refused(gpu):
    from wavernn_amd import _lib
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict
    sd, _ = block_prune_state_dict(random_state_dict(WSEED, compute_dims=8, res_blocks=1, mode='MOL'), 0.95, linear=True)
    eng = LoopEngine(sd, 'MOL', device=gpu)
    assert eng.tile_sparse_view()[0] == 0 and eng.sparse_blocks > 0
    with pytest.raises(_lib.WrnnError, match='wrnn_tile_sparse_kernel runs generic packs only'):
        eng.plan(16, T, algo='tile_sparse')
    assert eng.plan(16, T)['kernel'] == 'wrnn_sparse_kernel'


def test_model_score_with_loop_algo_tile_sparse(gpu):
    """`WaveRNN.score` with `loop_algo = 'tile_sparse'` on P1's model equals `loop_algo = 'tile'` within the bound tests/test_gpu_score.py holds two kernels
    on one model to, and the model names the kernel that ran."""
    from test_gpu_score import bound_of, short_wave
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel
    hp = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(5, 5, 11), feat_dims=80, compute_dims=8, res_out_dims=128, res_blocks=1,
              hop_length=275, sample_rate=22050)
    model = WaveRNN(**hp, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in _weights('P1').items()}, strict=True)
    model = model.to(gpu)
    mel, wav = torch.from_numpy(random_mel(140, 3)).unsqueeze(0), short_wave(3 * 275)
    res = {}
    for algo, kernel in (('tile_sparse', SPARSE), ('tile', TILE)):
        model.loop_algo = algo
        res[algo] = model.score(mel, wav, per_step=True)
        assert model.last_loop_kernel == kernel, (algo, model.last_loop_kernel)
    a, b = res['tile_sparse']['per_step'], res['tile']['per_step']
    assert a.shape == b.shape == (825,) and np.isfinite(a).all()
    err = float(np.abs(a - b).max())
    print(f'max per-step |tile_sparse - tile| = {err:.3e} (bound {bound_of("MOL"):.3e})')
    assert err <= bound_of('MOL')
