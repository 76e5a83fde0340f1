"""CPU tests of WRNN_ALGO_TILE_SPARSE = 12 in the launch planner (make_plan + ws_layout of csrc/wrnn_abi.hip), through `wrnn_debug_plan` on hand-written
traits, in the manner of tests/test_tile_plan.py: `wrnn_tile_sparse_kernel` (csrc/wrnn_tile_sparse.hip) is planned on request only, for generic packs that
carry a tile-sparse view (traits of a generic pack: sp_nbp > 0, sp_fc = 1 with fc1 / fc2) and whose activations fit wrnn_tile_kernel's LDS carve, with the
workspace `auto` gets for the same pack; everything else is refused with a text that says why.  No HIP device is needed."""
import os

import pytest

from test_planner_table import ERR_ARG, L, debug_plan      # noqa: F401  (L: the library fixture)
from test_tile_plan import GENERIC, SHIPPED, tile_lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, TILE_SPARSE = 10, 12
NAME = 'wrnn_tile_sparse_kernel'
VIEW = dict(GENERIC, sp_nbp=1)                  # a generic pack with the GRU view
VIEW_FC = dict(GENERIC, sp_nbp=1, sp_fc=1)      # ... and the fc view


def no_view(matrix, permille):
    """sp_nbp of a generic pack whose GRU matrix `matrix` keeps `permille` / 1000 of its blocks (include/wavernn_amd.h, wrnn_plan_traits)."""
    return -(1 + 1001 * matrix + permille)


def test_the_algo_has_a_name():
    from wavernn_amd._lib import ALGOS
    assert ALGOS['tile_sparse'] == TILE_SPARSE and ALGOS['tile'] == TILE


@pytest.mark.parametrize('traits', [VIEW, VIEW_FC], ids=['gru', 'gru_fc'])
@pytest.mark.parametrize('n_cus', [32, 256])
@pytest.mark.parametrize('noise_lib', [0, 1])
def test_a_pack_with_a_view_is_planned_onto_the_tile_sparse_kernel_with_autos_workspace(L, traits, n_cus, noise_lib):
    tr = dict(traits, n_cus=n_cus)
    for n in (1, 16, 17, 4096):
        for T in (100, 2000):
            rc, pl = debug_plan(L, tr, n, T, algo=TILE_SPARSE, noise_lib=noise_lib)
            assert rc == 0, pl
            assert (pl['kernel'], pl['rounds'], pl['slab_steps'], pl['clusters'], pl['depth'], pl['units_per_wg']) == (NAME, 1, T, 0, 0, 16), (n, T, pl)
            rc, auto = debug_plan(L, tr, n, T, algo=0, noise_lib=noise_lib)
            assert rc == 0 and auto['kernel'] == 'wrnn_generic_kernel'
            assert pl['workspace_bytes'] == auto['workspace_bytes'] > 0, (n, T, pl, auto)
            # `tile` on the same pack: as before
            rc, tile = debug_plan(L, tr, n, T, algo=TILE, noise_lib=noise_lib)
            assert rc == 0 and tile['kernel'] == 'wrnn_tile_kernel' and tile['workspace_bytes'] == auto['workspace_bytes']


@pytest.mark.parametrize('name', list(SHIPPED))
@pytest.mark.parametrize('n_cus', [32, 256])
def test_a_pack_of_the_shipped_dims_is_refused(L, name, n_cus):
    rc, msg = debug_plan(L, dict(SHIPPED[name], n_cus=n_cus), 16, 100, algo=TILE_SPARSE)
    assert rc == ERR_ARG and NAME in msg and 'generic packs only' in msg, msg


def test_a_generic_pack_without_a_view_is_refused_with_the_matrix_and_its_fraction(L):
    for m, name in enumerate(('rnn1.weight_ih', 'rnn1.weight_hh', 'rnn2.weight_ih', 'rnn2.weight_hh')):
        rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, sp_nbp=no_view(m, 537)), 16, 100, algo=TILE_SPARSE)
        assert rc == ERR_ARG and NAME in msg and 'no tile-sparse view' in msg and name in msg and '53.7 %' in msg and '41 %' in msg, msg
    # a dense pack: everything survives
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, sp_nbp=no_view(0, 1000)), 16, 100, algo=TILE_SPARSE)
    assert rc == ERR_ARG and 'rnn1.weight_ih' in msg and '100.0 %' in msg, msg
    # traits that record nothing
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256), 16, 100, algo=TILE_SPARSE)
    assert rc == ERR_ARG and NAME in msg and 'no tile-sparse view' in msg, msg
    # rnn no multiple of 16: the dim is named
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, gH=260), 16, 100, algo=TILE_SPARSE)
    assert rc == ERR_ARG and NAME in msg and 'rnn 260 is no multiple of 16' in msg, msg


def test_dims_past_the_lds_limit_are_refused_with_the_bytes_needed(L):
    rc, msg = debug_plan(L, dict(VIEW_FC, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE_SPARSE)
    need = tile_lds_bytes(2048, 2048, 80, 32)
    assert rc == ERR_ARG and NAME in msg and f'{need} bytes of LDS' in msg and str(160 * 1024) in msg, msg
    # `tile`'s text with the new kernel's name
    rc_t, msg_t = debug_plan(L, dict(VIEW_FC, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE)
    assert rc_t == ERR_ARG and msg == msg_t.replace('wrnn_tile_kernel', NAME)
    assert debug_plan(L, dict(VIEW_FC, n_cus=256, gH=576, gF=576), 16, 100, algo=TILE_SPARSE)[0] == 0
    assert debug_plan(L, dict(VIEW_FC, n_cus=256, gH=640, gF=640), 16, 100, algo=TILE_SPARSE)[0] == ERR_ARG


def test_a_step_range_and_two_sparse_groups_are_refused(L):
    tr = dict(VIEW, n_cus=256)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE_SPARSE, t_begin=10, t_end=60)
    assert rc == ERR_ARG and 'partial step range' in msg, msg
    assert (rc, msg) == debug_plan(L, tr, 16, 100, algo=TILE, t_begin=10, t_end=60)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE_SPARSE, sparse_groups=2)
    assert rc == ERR_ARG and f'this call runs on {NAME}' in msg, msg


def test_the_other_algo_values_answer_as_before(L):
    for tr in (dict(GENERIC, n_cus=256), dict(VIEW_FC, n_cus=256), dict(GENERIC, n_cus=256, sp_nbp=no_view(2, 800))):
        for algo in (3, 4, 9, 11):
            for traits in (tr, dict(SHIPPED['dense_mol'], n_cus=256)):
                assert debug_plan(L, traits, 16, 100, algo=algo) == (ERR_ARG, f'unknown algo {algo}')
        for algo in (2, 5, 6, 7, 8):
            rc, msg = debug_plan(L, tr, 16, 100, algo=algo)
            assert rc == ERR_ARG and msg.endswith('only the generic kernel (algo auto / stream) runs it'), msg
        for algo, kernel in ((0, 'wrnn_generic_kernel'), (1, 'wrnn_generic_kernel'), (TILE, 'wrnn_tile_kernel')):
            assert debug_plan(L, tr, 16, 100, algo=algo)[1]['kernel'] == kernel


def test_header_with_the_new_algo_is_plain_c(tmp_path):
    """As tests/test_host_logic.py::test_header_is_plain_c compiles it, with the new enumerator and the two new functions in use."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'use_header.c'
    src.write_text('#include "wavernn_amd.h"\n'
                   'int probe(const wrnn_pack *p, const float *w) {\n'
                   '    int32_t kept[6], total[6], tab[2], k, t, adm;\n'
                   '    return WRNN_ABI_VERSION + WRNN_ALGO_TILE_SPARSE + wrnn_pack_tile_sparse(p, kept, total)\n'
                   '           + wrnn_debug_tile_sparse_pack(w, 16, 4, 1, tab, 0, 0, 0, &k, &t, &adm);\n'
                   '}\n'
                   'typedef char tile_sparse_is_twelve[WRNN_ALGO_TILE_SPARSE == 12 ? 1 : -1];\n'
                   'typedef char tile_is_ten[WRNN_ALGO_TILE == 10 ? 1 : -1];\n'
                   'typedef char abi_is_nine[WRNN_ABI_VERSION == 9 ? 1 : -1];\n'
                   'typedef char traits_keep_their_size[sizeof(wrnn_plan_traits) == 48 ? 1 : -1];\n')
    res = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    from wavernn_amd import _lib
    assert _lib.lib().wrnn_abi_version() == 9 == _lib.ABI_VERSION
