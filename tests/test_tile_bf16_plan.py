"""CPU tests of WRNN_ALGO_TILE_BF16 = 13 in the launch planner (make_plan + ws_layout of csrc/wrnn_abi.hip), through `wrnn_debug_plan` on hand-written
traits, in the manner of tests/test_tile_sparse_plan.py: `wrnn_tile_bf16_kernel` (csrc/wrnn_tile_bf16.hip) is planned on request only, for generic packs
whose activations fit wrnn_tile_kernel's LDS carve (such a pack carries the bf16 view unless bit 1 of its sp_fc trait says that a weight rounded to
+-inf), with the workspace `auto` gets for the same pack; everything else is refused with `tile`'s texts under the new kernel's name.  No HIP device is
needed."""
import os

import pytest

from test_planner_table import ERR_ARG, L, debug_plan      # noqa: F401  (L: the library fixture)
from test_tile_plan import GENERIC, SHIPPED, tile_lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, TILE_SPARSE, TILE_BF16 = 10, 12, 13
NAME = 'wrnn_tile_bf16_kernel'
NO_VIEW = dict(GENERIC, sp_fc=2)                # a generic pack whose bf16 view was skipped


def test_the_algo_has_a_name():
    from wavernn_amd._lib import ALGOS
    assert ALGOS['tile_bf16'] == TILE_BF16 and ALGOS['tile'] == TILE and ALGOS['tile_sparse'] == TILE_SPARSE
    assert sorted(ALGOS.values()) == [0, 1, 2, 5, 6, 7, 8, 10, 12, 13]


@pytest.mark.parametrize('n_cus', [64, 256])
@pytest.mark.parametrize('noise_lib', [0, 1])
def test_a_generic_pack_is_planned_onto_the_bf16_kernel_with_autos_workspace(L, n_cus, noise_lib):
    for traits in (GENERIC, dict(GENERIC, mode=0, C=1024, gH=512, gF=512), dict(GENERIC, sp_nbp=1, sp_fc=1)):
        tr = dict(traits, n_cus=n_cus)
        for n in (1, 16, 17, 4096):
            for T in (100, 2000):
                rc, pl = debug_plan(L, tr, n, T, algo=TILE_BF16, noise_lib=noise_lib)
                assert rc == 0, pl
                assert (pl['kernel'], pl['rounds'], pl['slab_steps'], pl['clusters'], pl['depth'], pl['units_per_wg']) == (NAME, 1, T, 0, 0, 16), (n, T, pl)
                rc, auto = debug_plan(L, tr, n, T, algo=0, noise_lib=noise_lib)
                assert rc == 0 and auto['kernel'] == 'wrnn_generic_kernel'
                assert pl['workspace_bytes'] == auto['workspace_bytes'] > 0, (n, T, pl, auto)
                # `tile` on the same traits: as before
                rc, tile = debug_plan(L, tr, n, T, algo=TILE, noise_lib=noise_lib)
                assert rc == 0 and tile['kernel'] == 'wrnn_tile_kernel' and tile['workspace_bytes'] == auto['workspace_bytes']


@pytest.mark.parametrize('name', list(SHIPPED))
@pytest.mark.parametrize('n_cus', [64, 256])
def test_a_pack_of_the_shipped_dims_is_refused(L, name, n_cus):
    rc, msg = debug_plan(L, dict(SHIPPED[name], n_cus=n_cus), 16, 100, algo=TILE_BF16)
    assert rc == ERR_ARG and NAME in msg and 'generic packs only' in msg, msg
    rc_t, msg_t = debug_plan(L, dict(SHIPPED[name], n_cus=n_cus), 16, 100, algo=TILE)
    assert rc_t == ERR_ARG and msg == msg_t.replace('wrnn_tile_kernel', NAME)


def test_a_pack_without_a_view_is_refused(L):
    rc, msg = debug_plan(L, dict(NO_VIEW, n_cus=256), 16, 100, algo=TILE_BF16)
    assert rc == ERR_ARG and NAME in msg and 'no bf16 view' in msg and 'wrnn_pack_tile_bf16() == 0' in msg and 'inf' in msg, msg
    # ... and by nothing else
    for algo, kernel in ((0, 'wrnn_generic_kernel'), (TILE, 'wrnn_tile_kernel')):
        assert debug_plan(L, dict(NO_VIEW, n_cus=256), 16, 100, algo=algo)[1]['kernel'] == kernel
    # the tile-sparse fc bit beside it changes nothing
    assert debug_plan(L, dict(GENERIC, n_cus=256, sp_nbp=1, sp_fc=3), 16, 100, algo=TILE_BF16)[0] == ERR_ARG
    assert debug_plan(L, dict(GENERIC, n_cus=256, sp_nbp=1, sp_fc=3), 16, 100, algo=TILE_SPARSE)[1]['kernel'] == 'wrnn_tile_sparse_kernel'


def test_dims_past_the_lds_limit_are_refused_with_the_bytes_needed(L):
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE_BF16)
    need = tile_lds_bytes(2048, 2048, 80, 32)
    assert rc == ERR_ARG and NAME in msg and f'{need} bytes of LDS' in msg and str(160 * 1024) in msg, msg
    rc_t, msg_t = debug_plan(L, dict(GENERIC, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE)
    assert rc_t == ERR_ARG and msg == msg_t.replace('wrnn_tile_kernel', NAME)
    # (the LDS rule comes first: such a pack has no view either)
    assert debug_plan(L, dict(NO_VIEW, n_cus=256, gH=2048, gF=2048), 16, 100, algo=TILE_BF16) == (rc, msg)
    # rnn = fc = 512 and 576 at feat 80 / aux 32 are admitted, 640 is not
    for dims, want in ((512, 0), (576, 0), (640, ERR_ARG)):
        for mode, C in ((1, 30), (0, 1024)):
            assert debug_plan(L, dict(GENERIC, n_cus=256, mode=mode, C=C, gH=dims, gF=dims), 16, 100, algo=TILE_BF16)[0] == want, (dims, mode)
    assert tile_lds_bytes(576, 576, 80, 32) <= 160 * 1024 < tile_lds_bytes(640, 640, 80, 32)


def test_more_than_2048_raw_classes_are_refused(L):
    assert debug_plan(L, dict(GENERIC, n_cus=256, mode=0, C=2048), 16, 100, algo=TILE_BF16)[0] == 0
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256, mode=0, C=2049), 16, 100, algo=TILE_BF16)
    assert rc == ERR_ARG and NAME in msg and '<= 2048 classes' in msg, msg


def test_a_step_range_the_mel_stage_and_two_sparse_groups_are_refused(L):
    tr = dict(GENERIC, n_cus=256)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE_BF16, t_begin=10, t_end=60)
    assert rc == ERR_ARG and 'partial step range' in msg, msg
    assert (rc, msg) == debug_plan(L, tr, 16, 100, algo=TILE, t_begin=10, t_end=60)
    rc, msg = debug_plan(L, tr, 16, 100, algo=TILE_BF16, sparse_groups=2)
    assert rc == ERR_ARG and f'this call runs on {NAME}' in msg, msg


def test_the_kernel_forms_no_mel_stage():
    """wrnn_options.mel_stage is refused where the call is queued (the planner does not see it): the kernel's row of the per-kernel table has `tile`'s traits."""
    src = open(os.path.join(ROOT, 'wavernn_amd', 'csrc', 'wrnn_abi.hip')).read()
    row = [ln for ln in src.splitlines() if '"wrnn_tile_bf16_kernel"' in ln and 'K_TILE_BF16' in ln]
    tile = [ln for ln in src.splitlines() if '"wrnn_tile_kernel"' in ln and 'K_TILE ' in ln]
    assert len(row) == 1 and len(tile) == 1
    assert row[0].split('{')[1].replace('wrnn_tile_bf16_kernel', 'wrnn_tile_kernel') == tile[0].split('{')[1]


def test_the_other_algo_values_answer_as_before(L):
    for tr in (dict(GENERIC, n_cus=256), dict(NO_VIEW, n_cus=256)):
        for algo in (3, 4, 9, 11, 14):
            for traits in (tr, dict(SHIPPED['dense_mol'], n_cus=256)):
                assert debug_plan(L, traits, 16, 100, algo=algo) == (ERR_ARG, f'unknown algo {algo}')
        for algo in (2, 5, 6, 7, 8):
            rc, msg = debug_plan(L, tr, 16, 100, algo=algo)
            assert rc == ERR_ARG and msg.endswith('only the generic kernel (algo auto / stream) runs it'), msg
        for algo, kernel in ((0, 'wrnn_generic_kernel'), (1, 'wrnn_generic_kernel'), (TILE, 'wrnn_tile_kernel')):
            assert debug_plan(L, tr, 16, 100, algo=algo)[1]['kernel'] == kernel
    # `auto` never picks the new kernel
    for tr in (GENERIC, SHIPPED['dense_mol'], SHIPPED['raw256']):
        for n_cus in (32, 64, 256):
            for n in (1, 64, 1024):
                assert debug_plan(L, dict(tr, n_cus=n_cus), n, 100, algo=0)[1]['kernel'] != NAME


def test_header_with_the_new_algo_is_plain_c(tmp_path):
    """As tests/test_host_logic.py::test_header_is_plain_c compiles it, with the new enumerator and the two new functions in use."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'use_header.c'
    src.write_text('#include "wavernn_amd.h"\n'
                   'size_t probe(const wrnn_pack *p, const float *w, uint16_t *img) {\n'
                   '    return WRNN_ABI_VERSION + WRNN_ALGO_TILE_BF16 + wrnn_pack_tile_bf16(p) + (size_t)wrnn_debug_tile_bf16_pack(w, 16, 8, img, 2560);\n'
                   '}\n'
                   'typedef char tile_bf16_is_thirteen[WRNN_ALGO_TILE_BF16 == 13 ? 1 : -1];\n'
                   'typedef char tile_sparse_is_twelve[WRNN_ALGO_TILE_SPARSE == 12 ? 1 : -1];\n'
                   'typedef char tile_is_ten[WRNN_ALGO_TILE == 10 ? 1 : -1];\n'
                   'typedef char abi_is_nine[WRNN_ABI_VERSION == 9 ? 1 : -1];\n'
                   'typedef char traits_keep_their_size[sizeof(wrnn_plan_traits) == 48 ? 1 : -1];\n')
    res = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    from wavernn_amd import _lib
    assert _lib.lib().wrnn_abi_version() == 9 == _lib.ABI_VERSION
