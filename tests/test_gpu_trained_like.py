"""Every loop kernel on trained-like weights (tests/trained_like.py): saturated GRU gates, peaked RAW logits, MoL log-scales below the clamp and samples beyond
both clips -- the regime `synthetic.random_state_dict` never reaches, in which `sigmoid_f` / `tanh_sel` / the saturating branch of tanhf, exp() underflow in the RAW
samplers, the first-maximum rule among classes of probability 0, the `log_scale_min` clamp and the +-1 clips run.

One teacher-forced call per (case, kernel) through `LoopEngine.run_segments` with `force_x` and `want_logits=True` returns the kernel's logits AND the sample it
drew from exactly those logits (every loop kernel writes its own sample to `out` before it substitutes `force_x`).  Assertions per call
(`trained_like.check_call`):

  1. logits and samples are finite;
  2. max |Lk - L64| / (1 + max_c |L64|) <= 8 E_ref against the float64 loop (oracle/loop_f64.py), E_ref = what the float32 reference arithmetic loses on the
     same case (plain and permuted summation order), recomputed here from the memoised oracle runs.  Why 8: a kernel's MFMA summation order is another draw of
     the same rounding noise pushed through the same Jacobians -- on the CPU the permuted order lands at 0.4-1.4 x the plain one -- while what this test exists
     for (a wrong clamp, an overflowing activation, a dropped bias) shows at 1e-3 or as NaN.  The factor is fixed;
  3. RAW: `out` is `wavernn_oracle.sample_raw` on the kernel's own logits, except at near-ties of the two best float64 p / q (either of the two; share <= 0.5 %);
  4. MoL: |out - clip(x64, -1, 1)| <= 8 E_samp m with the float64 argmax component (a gumbel near-tie: or the second-best; share <= 0.5 %), beyond the clips
     exactly +-1, and the clamp, the -1 clip and the +1 clip each ran on this kernel's logits.

No sample equality against an oracle TRAJECTORY is asserted here: off the linear regime the loop amplifies rounding differences, and a correct kernel leaves the
float32 oracle's trajectory.  What does not care about chaos is bit-identity between kernels that promise it: the free-running tests at the end.

tests/test_trained_like_host.py holds every case used here to its conditions on the CPU.  wrnn_sparse_kernel's two-groups form is a MoL form: RAW has none."""
import numpy as np
import pytest
import torch

import trained_like as TL

pytestmark = pytest.mark.gpu

_MEMO = {}
KERNEL = {'stream': 'wrnn_stream_kernel', 'loop': 'wrnn_loop_kernel', 'duo': 'wrnn_duo_kernel', 'chain': 'wrnn_chain_kernel', 'octo': 'wrnn_octo_kernel',
          'sparse': 'wrnn_sparse_kernel', 'generic': 'wrnn_generic_kernel', 'tile': 'wrnn_tile_kernel', 'tile_wide': 'wrnn_tile_wide_kernel',
          'tile_bf16': 'wrnn_tile_bf16_kernel', 'tile_sparse': 'wrnn_tile_sparse_kernel'}
SLAB = 23                      # 64 steps in slabs of 23: saturated state crosses a slab save and restore twice


def _has_octo():
    from wavernn_amd import _lib
    return 'octo' in _lib.ALGOS


def _calls():
    """(id, case, kernel, run_segments options) of every teacher-forced call."""
    out = []
    for mode in ('mol', 'raw'):
        for k in ('stream', 'loop', 'duo', 'chain') + (('octo',) if mode == 'mol' and _has_octo() else ()):
            out.append((f'ship_{mode}-{k}', f'ship_{mode}', k, dict(algo=k)))
        for k in ('loop', 'duo', 'chain'):
            out.append((f'ship_{mode}-{k}-slabs', f'ship_{mode}', k, dict(algo=k, slab_steps=SLAB)))
        out.append((f'ship_pruned_{mode}-sparse', f'ship_pruned_{mode}', 'sparse', dict(algo='sparse')))
    out.append(('ship_pruned_mol-sparse-two-groups', 'ship_pruned_mol', 'sparse', dict(algo='sparse', sparse_groups=2)))
    for d in ('d256_mol', 'd144_raw'):
        out += [(f'{d}-generic', d, 'generic', dict(algo='auto')), (f'{d}-tile', d, 'tile', dict(algo='tile')),
                (f'{d}-tile-w4', d, 'tile_wide', dict(algo='tile', clusters=4)), (f'{d}-tile_bf16', d + '_bf16', 'tile_bf16', dict(algo='tile_bf16')),
                (f'{d}-tile_sparse', d + '_pruned', 'tile_sparse', dict(algo='tile_sparse'))]
    out += [('g520_raw-generic', 'g520_raw', 'generic', dict(algo='auto')), ('g100_raw1-generic', 'g100_raw1', 'generic', dict(algo='auto'))]
    return out


CALLS = _calls()


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    from wavernn_amd import _lib
    _lib.lib()
    return torch.device('cuda', 0)


def _engine(gpu, name):
    """One engine per case (its mode is the case's), shared by the kernels run on it."""
    if ('engine', name) not in _MEMO:
        from wavernn_amd.engine import LoopEngine
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')          # (a pruned 9-bit RAW pack says once that `auto` would run it dense: every call here names its kernel)
            _MEMO[('engine', name)] = LoopEngine(TL.weights(name), TL.inputs(name)['mode'], device=gpu)
    return _MEMO[('engine', name)]


def _run(gpu, name, kernel, opts, c=None, forced=True, want_logits=True):
    """One `run_segments` call of case `name` (c: its inputs; default the teacher-forced case) -> (out [B, T], logits [T, B, C]) as host arrays."""
    c = TL.case(name) if c is None else c
    key = ('dev', name, c['T'])
    if key not in _MEMO:
        _MEMO[key] = tuple(torch.from_numpy(c[k]).to(gpu) for k in ('mels_up', 'aux', 'flat'))
    mels_up, aux, flat = _MEMO[key]
    kw = dict(opts, want_logits=want_logits)
    if forced:
        kw['force_x'] = torch.from_numpy(c['force_x'])
    eng = _engine(gpu, name)
    res = eng.run_segments(mels_up, aux, c['seg_pos'], c['seg_lim'], c['T'], flat, c['hop'], **kw)
    assert eng.last_loop_kernel() == KERNEL[kernel], (name, kernel, eng.last_loop_kernel())
    return tuple(r.cpu().numpy() for r in res) if want_logits else res.cpu().numpy()


@pytest.mark.parametrize('label, name, kernel, opts', CALLS, ids=[c[0] for c in CALLS])
def test_teacher_forced_call(gpu, label, name, kernel, opts):
    """Assertions 1-4 of the module docstring on one kernel's teacher-forced call."""
    c = TL.case(name)
    assert 0 < c['e_ref'] <= TL.E_REF_MAX, (name, c['e_ref'])            # (the case is a valid input: tests/test_trained_like_host.py)
    out, Lk = _run(gpu, name, kernel, opts)
    assert out.shape == (c['B'], c['T']) and Lk.shape == c['L64'].shape
    res = TL.check_call(out, Lk, c, label)
    print(f'{label}: sampler {res}')


# ---- free-running bit-identity: what the kernels promise one another, on trained-like weights and the same noise, T = 64 ---------------------------------
def _free(gpu, name, kernel, opts, want_logits=True):
    key = ('free', name, kernel, tuple(sorted(opts.items())), want_logits)
    if key not in _MEMO:
        _MEMO[key] = _run(gpu, name, kernel, opts, c=TL.inputs(name, T=64), forced=False, want_logits=want_logits)
    return _MEMO[key]


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert bad.size == 0, f'{what}: {len(bad)} of {a.size} values differ in their bits, first at {tuple(bad[0])}'
    assert np.isfinite(a).all() and len(np.unique(a)) > 1


#: wrnn_chain_kernel runs wrnn_duo_kernel's stage arithmetic -- except that a MoL call with ONE slot per cluster folds fc3 into the fc2 stage (DESIGN.md section 3,
#: K-chain (4): the same products in another summation order, so not the same bits; 40 segments are three groups on three clusters, one slot each).  For MoL the
#: identity is the unfolded form's (tuning bit 4).
CHAIN_FORMS = [('ship_raw', {}), ('ship_mol', dict(tuning=16))]


@pytest.mark.parametrize('name, form', CHAIN_FORMS, ids=[n + ''.join(f'-{k}{v}' for k, v in f.items()) for n, f in CHAIN_FORMS])
def test_chain_samples_are_duo_samples(gpu, name, form):
    duo = _free(gpu, name, 'duo', dict(algo='duo'), want_logits=False)
    _same(_free(gpu, name, 'chain', dict(algo='chain', **form), want_logits=False), duo, f'{name}: chain {form} vs duo samples')


@pytest.mark.parametrize('W', [2, 4, 8])
@pytest.mark.parametrize('name', ['d256_mol', 'd144_raw'])
def test_wide_tile_is_tile(gpu, name, W):
    out, lg = _free(gpu, name, 'tile', dict(algo='tile'))
    w_out, w_lg = _free(gpu, name, 'tile_wide', dict(algo='tile', clusters=W))
    _same(w_out, out, f'{name} W = {W}: samples vs wrnn_tile_kernel')
    _same(w_lg, lg, f'{name} W = {W}: logits vs wrnn_tile_kernel')


@pytest.mark.parametrize('name', ['d256_mol_pruned', 'd144_raw_pruned'])
def test_tile_sparse_logits_are_tile_logits_on_the_masked_weights(gpu, name):
    out, lg = _free(gpu, name, 'tile', dict(algo='tile'))
    s_out, s_lg = _free(gpu, name, 'tile_sparse', dict(algo='tile_sparse'))
    _same(s_lg, lg, f'{name}: logits vs wrnn_tile_kernel on the masked weights')
    _same(s_out, out, f'{name}: samples vs wrnn_tile_kernel on the masked weights')
