"""CPU tests of WRNN_ALGO_TILE = 10 in the launch planner (make_plan + ws_layout of csrc/wrnn_abi.hip), through `wrnn_debug_plan` on hand-written traits:
`wrnn_tile_kernel` (csrc/wrnn_tile.hip) is planned on request only, for generic packs whose activations fit its LDS carve, with the workspace `auto` gets
for the same pack (status words, segment table, and all T steps of the library's noise when it draws it); everything else is refused with a text that
says why.  No HIP device is needed."""
import os

import pytest

from test_planner_table import ERR_ARG, L, debug_plan      # noqa: F401  (L: the library fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 10
GENERIC = dict(mode=1, C=30, generic=1, gH=256, gF=256, gM=80, gA=32, sp_max_blocks=256)
#: the packs of scripts/make_golden.py that are NOT generic
SHIPPED = dict(dense_mol=dict(mode=1, C=30, sp_max_blocks=512), raw256=dict(mode=0, C=256, sp_max_blocks=512),
               sparse_mol_48=dict(mode=1, C=30, sp_nbp=48, sp_max_blocks=40))
#: the geometries of tests/test_gpu_tile.py (mode, C, rnn, fc, feat, aux) and the 10-bit model at the shipped dims
GPU_CASES = dict(T1=(0, 1024, 520, 257, 13, 5), T2=(0, 1024, 72, 600, 80, 32), T3=(0, 2, 100, 50, 7, 1), T4=(1, 30, 260, 33, 3, 3),
                 T5=(1, 30, 256, 256, 80, 32), raw10=(0, 1024, 512, 512, 80, 32))


def tile_lds_bytes(H, F, M, A):
    """The LDS rule of include/wavernn_amd.h (WRNN_ALGO_TILE), restated."""
    def up4(n):
        return (n + 3) // 4 * 4
    return 16 * 4 * (up4(1 + M + A) + 2 * up4(max(H, F) + A) + 2 * up4(H)) + 2560


def test_the_algo_has_a_name():
    from wavernn_amd._lib import ALGOS
    assert ALGOS['tile'] == TILE


@pytest.mark.parametrize('n_cus', [32, 256])
@pytest.mark.parametrize('noise_lib', [0, 1])
def test_a_generic_pack_is_planned_onto_the_tile_kernel_with_autos_workspace(L, n_cus, noise_lib):
    tr = dict(GENERIC, n_cus=n_cus)
    for n in (1, 16, 17, 4096):
        for T in (100, 2000):
            rc, pl = debug_plan(L, tr, n, T, algo=TILE, noise_lib=noise_lib)
            assert rc == 0, pl
            assert (pl['kernel'], pl['rounds'], pl['slab_steps'], pl['clusters'], pl['depth']) == ('wrnn_tile_kernel', 1, T, 0, 0), (n, T, pl)
            rc, auto = debug_plan(L, tr, n, T, algo=0, noise_lib=noise_lib)
            assert rc == 0 and auto['kernel'] == 'wrnn_generic_kernel'
            assert pl['workspace_bytes'] == auto['workspace_bytes'] > 0, (n, T, pl, auto)
    # the library's noise: all T steps of it join the workspace
    if noise_lib:
        assert debug_plan(L, tr, 17, 100, algo=TILE, noise_lib=1)[1]['workspace_bytes'] - debug_plan(L, tr, 17, 100, algo=TILE)[1]['workspace_bytes'] \
            >= 100 * 17 * 11 * 4


@pytest.mark.parametrize('name', list(GPU_CASES))
def test_the_lds_rule_takes_the_tested_geometries(L, name):
    mode, C, H, F, M, A = GPU_CASES[name]
    assert tile_lds_bytes(H, F, M, A) <= 160 * 1024
    rc, pl = debug_plan(L, dict(n_cus=256, mode=mode, C=C, generic=1, gH=H, gF=F, gM=M, gA=A, sp_max_blocks=H), 17, 64, algo=TILE)
    assert rc == 0 and pl['kernel'] == 'wrnn_tile_kernel', pl


@pytest.mark.parametrize('name', list(SHIPPED))
@pytest.mark.parametrize('n_cus', [32, 256])
def test_a_pack_of_the_shipped_dims_is_refused(L, name, n_cus):
    rc, msg = debug_plan(L, dict(SHIPPED[name], n_cus=n_cus), 16, 100, algo=TILE)
    assert rc == ERR_ARG and 'wrnn_tile_kernel' in msg and 'generic packs only' in msg, msg


def test_dims_past_the_lds_limit_are_refused_with_the_bytes_needed(L):
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE)
    need = tile_lds_bytes(2048, 2048, 80, 32)
    assert rc == ERR_ARG and 'wrnn_tile_kernel' in msg and f'{need} bytes of LDS' in msg and str(160 * 1024) in msg, msg
    # either side of the limit (rnn = fc, feat 80, aux 32): 576 fits, 640 does not
    assert tile_lds_bytes(576, 576, 80, 32) <= 160 * 1024 < tile_lds_bytes(640, 640, 80, 32)
    assert debug_plan(L, dict(GENERIC, n_cus=256, gH=576, gF=576), 16, 100, algo=TILE)[0] == 0
    assert debug_plan(L, dict(GENERIC, n_cus=256, gH=640, gF=640), 16, 100, algo=TILE)[0] == ERR_ARG
    # `auto` is unchanged: the generic kernel takes them
    assert debug_plan(L, dict(GENERIC, n_cus=256, gH=640, gF=640), 16, 100)[1]['kernel'] == 'wrnn_generic_kernel'


def test_a_step_range_and_two_sparse_groups_are_refused_as_on_the_generic_kernel(L):
    tr = dict(GENERIC, n_cus=256)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE, t_begin=10, t_end=60)
    assert rc == ERR_ARG and 'partial step range' in msg, msg
    assert (rc, msg) == debug_plan(L, tr, 16, 100, algo=0, t_begin=10, t_end=60)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE, sparse_groups=2)
    assert rc == ERR_ARG and 'this call runs on wrnn_tile_kernel' in msg, msg


def test_the_other_algo_values_answer_as_before(L):
    tr = dict(GENERIC, n_cus=256)
    for algo in (3, 4, 9, 11):
        for traits in (tr, dict(SHIPPED['dense_mol'], n_cus=256)):
            assert debug_plan(L, traits, 16, 100, algo=algo) == (ERR_ARG, f'unknown algo {algo}')
    for algo in (2, 5, 6, 7, 8):
        rc, msg = debug_plan(L, tr, 16, 100, algo=algo)
        assert rc == ERR_ARG and msg.endswith('only the generic kernel (algo auto / stream) runs it'), msg


def test_header_with_the_new_algo_is_plain_c(tmp_path):
    """As tests/test_host_logic.py::test_header_is_plain_c compiles it, with the new enumerator in use."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'use_header.c'
    src.write_text('#include "wavernn_amd.h"\n'
                   'int probe(void) { wrnn_options o; (void)o; return WRNN_ABI_VERSION + WRNN_ALGO_TILE + WRNN_ALGO_SPARSE; }\n'
                   'typedef char tile_is_ten[WRNN_ALGO_TILE == 10 ? 1 : -1];\n'
                   'typedef char abi_is_nine[WRNN_ABI_VERSION == 9 ? 1 : -1];\n')
    res = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
