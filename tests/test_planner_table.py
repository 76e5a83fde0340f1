"""CPU tests of the launch planner (make_plan + ws_layout of csrc/wrnn_abi.hip) through `wrnn_debug_plan`, which plans for a
hand-written description of pack and device: no HIP device is needed, and device sizes nobody has are planned for as well.

tests/golden/planner_table.npz (`python scripts/make_golden.py planner_table`) was recorded from the planner before it was restructured
around one per-kernel table: whatever it answered then -- kernel, split, rounds, slab length, workspace bytes, return code, error text --
it must answer now."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN

ERR_ARG, ERR_RESIDENCY = -1, -6
KERNELS = ('wrnn_stream_kernel', 'wrnn_generic_kernel', 'wrnn_loop_kernel', 'wrnn_duo_kernel', 'wrnn_chain_kernel', 'wrnn_sparse_kernel',
           'wrnn_octo_kernel')


@pytest.fixture(scope='module')
def L():
    from wavernn_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def debug_plan(L, traits, n_segments, T, n_frames=700, **opts):
    """wrnn_debug_plan -> (rc, dict(kernel, units_per_wg, clusters, depth, rounds, slab_steps, workspace_bytes) or the error text)."""
    from wavernn_amd import _lib
    t, o, i, ws = _lib.PlanTraits(**traits), _lib.Options(**opts), _lib.RunInfo(), ctypes.c_size_t(0)
    rc = L.wrnn_debug_plan(ctypes.byref(t), n_segments, T, n_frames, ctypes.byref(o), ctypes.byref(i), ctypes.byref(ws))
    if rc != 0:
        return rc, L.wrnn_last_error().decode()
    return rc, dict(kernel=i.kernel.decode(), units_per_wg=i.units_per_wg, clusters=i.clusters, depth=i.depth, rounds=i.rounds,
                    slab_steps=i.slab_steps, workspace_bytes=ws.value)


def test_every_row_of_the_recorded_table_is_reproduced(L):
    g = np.load(os.path.join(GOLDEN, 'planner_table.npz'))
    tnames, cnames, onames = list(g['trait_names']), list(g['call_names']), list(g['out_names'])
    assert onames == ['rc', 'kernel', 'units_per_wg', 'clusters', 'depth', 'rounds', 'slab_steps', 'workspace_bytes', 'error']
    kernels, errors = list(g['kernels']), list(g['errors'])
    assert len(g['traits']) == len(g['call']) == len(g['out']) > 20000
    bad = []
    for n, (tr, call, out) in enumerate(zip(g['traits'].tolist(), g['call'].tolist(), g['out'].tolist())):
        c = dict(zip(cnames, call))
        rc, got = debug_plan(L, dict(zip(tnames, tr)), c['n_segments'], c['T'], c['n_frames'], algo=c['algo'], depth=c['depth'],
                             clusters=c['clusters'], slab_steps=c['slab_steps'], t_begin=c['t_begin'], t_end=c['t_end'])
        want = dict(zip(onames, out))
        if want['rc'] != 0:
            ok = rc == want['rc'] and got == errors[want['error']]
        else:
            ok = rc == 0 and got == dict(kernel=kernels[want['kernel']], **{k: want[k] for k in onames[2:8]})
        if not ok:
            bad.append((n, dict(zip(tnames, tr)), c, want, rc, got))
    assert not bad, f'{len(bad)} rows differ; the first: {bad[0]}'


def test_the_recorded_table_covers_the_planner():
    """Every kernel is planned somewhere, both refusals occur, and every device size but the smallest (stream kernel only) is planned
    onto at least two different cluster counts."""
    g = np.load(os.path.join(GOLDEN, 'planner_table.npz'))
    out, cus = g['out'], g['traits'][:, list(g['trait_names']).index('n_cus')]
    ok = out[:, 0] == 0
    assert {str(g['kernels'][k]) for k in np.unique(out[ok, 1])} == set(KERNELS)
    assert {ERR_ARG, ERR_RESIDENCY} <= set(out[:, 0].tolist()) and set(out[:, 0].tolist()) <= {0, ERR_ARG, ERR_RESIDENCY}
    assert sorted(set(cus.tolist())) == [32, 64, 128, 192, 255, 256, 304]
    for n in sorted(set(cus.tolist())):
        rows = ok & (cus == n)
        clusters = set(out[rows, 3].tolist())
        if n == 32:
            assert {str(g['kernels'][k]) for k in np.unique(out[rows, 1])} == {'wrnn_stream_kernel', 'wrnn_generic_kernel'} and clusters == {0}
        else:
            assert len(clusters) >= 2, (n, clusters)


def test_planner_picks_the_kernel_by_pack_and_batch_on_256_cus(L):
    """The cases of tests/test_gpu_parity.py::test_planner_picks_the_kernel_by_pack_and_batch, on a described 256-CU device."""
    dense = dict(n_cus=256, mode=1, C=30, sp_max_blocks=512)
    raw = dict(n_cus=256, mode=0, C=512, sp_max_blocks=512)
    raw8 = dict(n_cus=256, mode=0, C=256, sp_max_blocks=512)
    sparse = dict(n_cus=256, mode=1, C=30, sp_nbp=48, sp_max_blocks=40, sp_fc=0)
    from wavernn_amd._lib import ALGOS

    def plan(tr, n, T, algo='auto', n_frames=700):
        rc, got = debug_plan(L, tr, n, T, n_frames, algo=ALGOS[algo])
        assert rc == 0, got
        return got

    def refusal(tr, n, T, algo):
        rc, got = debug_plan(L, tr, n, T, algo=ALGOS[algo])
        assert rc == ERR_ARG
        return got

    for n, kernel, depth in ((1, 'wrnn_chain_kernel', 1), (12, 'wrnn_chain_kernel', 1), (64, 'wrnn_chain_kernel', 1), (65, 'wrnn_chain_kernel', 2),
                             (128, 'wrnn_chain_kernel', 2), (129, 'wrnn_duo_kernel', 3), (256, 'wrnn_duo_kernel', 4), (512, 'wrnn_duo_kernel', 8)):
        pl = plan(dense, n, 12100)
        assert (pl['kernel'], pl['clusters'], pl['depth'], pl['rounds']) == (kernel, 4, depth, 1), (n, pl)
    assert plan(dense, 256, 12100, 'chain')['depth'] == 4 and plan(dense, 300, 12100, 'chain')['rounds'] == 2
    assert plan(dense, 256, 12100, 'octo') == dict(plan(dense, 256, 12100, 'duo'), kernel='wrnn_octo_kernel')
    assert (plan(dense, 512, 12100, 'octo')['depth'], plan(dense, 512, 12100, 'octo')['rounds']) == (4, 2)
    assert 'block-sparse kernel needs' in refusal(dense, 16, 100, 'sparse')
    assert plan(raw, 12, 12100)['kernel'] == 'wrnn_chain_kernel' and plan(raw, 128, 12100)['depth'] == 2 and plan(raw, 256, 12100)['kernel'] == 'wrnn_duo_kernel'
    assert plan(raw8, 12, 100)['kernel'] == 'wrnn_stream_kernel'
    assert 'wrnn_chain_kernel needs MOL or RAW with 512 classes' in refusal(raw8, 12, 100, 'chain')
    assert 'wrnn_octo_kernel needs MOL' in refusal(raw, 256, 12100, 'octo')
    for n, rounds in ((12, 1), (256, 1), (257, 2), (942, 4)):
        pl = plan(sparse, n, 12100)
        assert (pl['kernel'], pl['units_per_wg'], pl['clusters'], pl['depth'], pl['rounds']) == ('wrnn_sparse_kernel', 64, 16, 1, rounds), (n, pl)
    assert plan(sparse, 256, 12100, 'duo')['kernel'] == 'wrnn_duo_kernel' and plan(sparse, 12, 12100, 'chain')['kernel'] == 'wrnn_chain_kernel'
    for tr, n in ((dense, 12), (sparse, 256)):
        assert plan(tr, n, 12100, n_frames=700)['workspace_bytes'] == plan(tr, n, 121000, n_frames=70000)['workspace_bytes'] < 300e6
