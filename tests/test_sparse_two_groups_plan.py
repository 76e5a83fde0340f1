"""CPU tests of the launch planner for wrnn_options.sparse_groups (two groups of <= 16 segments per cluster of wrnn_sparse_kernel, on request), through
`wrnn_debug_plan` on hand-written traits: a 256-CU device, a MoL pack whose GRU matrices and Linear layers are block-sparse."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN
from test_planner_table import ERR_ARG, ERR_RESIDENCY, L, debug_plan      # noqa: F401  (L: the library fixture)

MOL, RAW = 1, 0
ALGO_AUTO, ALGO_SPARSE, ALGO_DUO = 0, 5, 6


def traits(nbp=48, **kw):
    t = dict(n_cus=256, mode=MOL, C=30, generic=0, gH=512, gF=512, gM=80, gA=32, sp_nbp=nbp, sp_max_blocks=nbp - 7, sp_fc=1)
    t.update(kw)
    return t


@pytest.mark.parametrize('nbp', [48, 64])
@pytest.mark.parametrize('algo', [ALGO_AUTO, ALGO_SPARSE])
def test_two_groups_plan_depth_two_and_32_groups_a_round(L, nbp, algo):
    for n, rounds in ((12, 1), (256, 1), (257, 1), (512, 1), (513, 2), (942, 2)):
        rc, pl = debug_plan(L, traits(nbp), n, 12100, algo=algo, sparse_groups=2)
        assert rc == 0, pl
        assert (pl['kernel'], pl['units_per_wg'], pl['clusters'], pl['depth'], pl['rounds']) == ('wrnn_sparse_kernel', 64, 16, 2, rounds), (n, pl)
        # wrnn_options.depth still does not apply to this kernel
        assert debug_plan(L, traits(nbp), n, 12100, algo=algo, sparse_groups=2, depth=1) == (rc, pl)
        assert debug_plan(L, traits(nbp), n, 12100, algo=algo, sparse_groups=2, depth=4) == (rc, pl)


def test_two_groups_workspace_holds_512_segments_a_round_whatever_T(L):
    for nbp in (48, 64):
        for n in (12, 512, 942):
            a = debug_plan(L, traits(nbp), n, 12100, n_frames=700, sparse_groups=2)[1]
            b = debug_plan(L, traits(nbp), n, 121000, n_frames=7000, sparse_groups=2)[1]
            assert a['workspace_bytes'] == b['workspace_bytes'], (n, a, b)
        two = debug_plan(L, traits(nbp), 512, 12100, sparse_groups=2)[1]
        one = debug_plan(L, traits(nbp), 512, 12100)[1]
        assert two['workspace_bytes'] < 300e6
        # state and ring of 32 groups in one round instead of 2 rounds x 16 groups of state and 16 regions of ring: 16 more regions
        # (17 layers x 4 entries x 32 KB each), nothing else
        assert two['workspace_bytes'] - one['workspace_bytes'] == 16 * 17 * 4 * 32768, (one, two)


def test_one_group_answers_are_the_recorded_ones(L):
    """sparse_groups = 0, = 1, and an options struct that ends in front of the field: what the planner answered before the field existed
    (tests/golden/planner_table.npz, every row planned on a block-sparse pack)."""
    from wavernn_amd import _lib
    g = np.load(os.path.join(GOLDEN, 'planner_table.npz'))
    tnames, cnames, onames = list(g['trait_names']), list(g['call_names']), list(g['out_names'])
    kernels, errors = list(g['kernels']), list(g['errors'])
    rows = [(tr, call, out) for tr, call, out in zip(g['traits'].tolist(), g['call'].tolist(), g['out'].tolist()) if dict(zip(tnames, tr))['sp_nbp'] > 0]
    assert len(rows) > 500
    old_size = _lib.Options.sparse_groups.offset
    assert old_size < ctypes.sizeof(_lib.Options)
    seen_sparse = 0
    for tr, call, out in rows[::3]:
        c, want = dict(zip(cnames, call)), dict(zip(onames, out))
        kw = dict(algo=c['algo'], depth=c['depth'], clusters=c['clusters'], slab_steps=c['slab_steps'], t_begin=c['t_begin'], t_end=c['t_end'])
        expect = (want['rc'], errors[want['error']]) if want['rc'] != 0 else (0, dict(kernel=kernels[want['kernel']], **{k: want[k] for k in onames[2:8]}))
        seen_sparse += want['rc'] == 0 and kernels[want['kernel']] == 'wrnn_sparse_kernel'
        for groups in (0, 1):
            assert debug_plan(L, dict(zip(tnames, tr)), c['n_segments'], c['T'], c['n_frames'], sparse_groups=groups, **kw) == expect, (tr, c, groups)
        # a caller built against the header without the field: whatever lies behind its struct is not read
        t, o, i, ws = _lib.PlanTraits(**dict(zip(tnames, tr))), _lib.Options(sparse_groups=2, **kw), _lib.RunInfo(), ctypes.c_size_t(0)
        o.struct_bytes = old_size
        rc = L.wrnn_debug_plan(ctypes.byref(t), c['n_segments'], c['T'], c['n_frames'], ctypes.byref(o), ctypes.byref(i), ctypes.byref(ws))
        got = (rc, L.wrnn_last_error().decode()) if rc else (0, dict(kernel=i.kernel.decode(), units_per_wg=i.units_per_wg, clusters=i.clusters, depth=i.depth,
                                                                      rounds=i.rounds, slab_steps=i.slab_steps, workspace_bytes=ws.value))
        assert got == expect, (tr, c)
    assert seen_sparse > 50


def test_two_groups_refusals_say_why(L):
    def refused(tr, rc_want=ERR_ARG, n=512, **kw):
        rc, msg = debug_plan(L, tr, n, 12100, sparse_groups=kw.pop('sparse_groups', 2), **kw)
        assert rc == rc_want, (rc, msg)
        return msg
    for nbp in (48, 64):
        assert 'Linear layers are block-sparse too' in refused(traits(nbp, sp_fc=0))                       # dense fc tiles: no register room
        assert 'Linear layers are block-sparse too' in refused(traits(nbp), tuning=2048)                   # ... also when the A/B switch asks for them
        assert '9-bit RAW' in refused(traits(nbp, mode=RAW, C=512), algo=ALGO_SPARSE)
        assert 'sparse_groups = 3' in refused(traits(nbp), sparse_groups=3)
        assert 'sparse_groups = -1' in refused(traits(nbp), sparse_groups=-1)
        assert 'this call runs on wrnn_duo_kernel' in refused(traits(nbp), algo=ALGO_DUO)
        assert 'phase-clock build' in refused(traits(nbp), phase_clocks=1 << 20)
    dense = traits(sp_nbp=0, sp_max_blocks=512, sp_fc=0)
    assert 'this call runs on wrnn_duo_kernel' in refused(dense)                                          # a dense pack: `auto` plans the duo kernel
    assert 'this call runs on wrnn_chain_kernel' in refused(dense, n=12)
    assert 'this call runs on wrnn_duo_kernel' in refused(traits(mode=RAW, C=512))                        # a sparse RAW pack under `auto`: the dense kernels
    assert 'this call runs on wrnn_generic_kernel' in refused(traits(generic=1, gH=256))
    # fewer than 256 CUs: the kernel is not there to run two groups on
    assert '>= 256 CUs' in refused(traits(n_cus=128), rc_want=ERR_RESIDENCY, algo=ALGO_SPARSE)
    assert 'only wrnn_sparse_kernel runs two groups per cluster' in refused(traits(n_cus=128))
    # ... and none of it touches a call that leaves the field alone
    assert debug_plan(L, traits(sp_fc=0), 512, 12100)[0] == 0 and debug_plan(L, dense, 512, 12100, sparse_groups=1)[0] == 0
