"""CPU tests of the wide form of WRNN_ALGO_TILE in the launch planner (make_plan + ws_layout of csrc/wrnn_abi.hip), through `wrnn_debug_plan` on the traits of
tests/test_tile_plan.py: wrnn_options.clusters = 2, 4 or 8 under algo tile plans `wrnn_tile_wide_kernel` (csrc/wrnn_tile_wide.hip) -- that many workgroups per
tile of 16 segments, one round, at most one workgroup per CU --, 0 and 1 plan what they planned before, every refusal of tile keeps its text, and no other
algo learns a new meaning of the field.  No HIP device is needed."""
import ctypes
import os

import pytest

from test_planner_table import ERR_ARG, L, debug_plan      # noqa: F401  (L: the library fixture)
from test_tile_plan import GENERIC, SHIPPED, TILE, tile_lds_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = 'wrnn_tile_wide_kernel'
WIDTHS = (2, 4, 8)


@pytest.mark.parametrize('noise_lib', [0, 1])
def test_clusters_0_and_1_answer_exactly_as_tile_does_today(L, noise_lib):
    """Today's answer, restated from tests/test_tile_plan.py: wrnn_tile_kernel, `auto`'s workspace, one round, no clusters, no depth."""
    for n_cus in (32, 256):
        tr = dict(GENERIC, n_cus=n_cus)
        for n in (1, 16, 17, 4096):
            for T in (100, 2000):
                rc, auto = debug_plan(L, tr, n, T, algo=0, noise_lib=noise_lib)
                assert rc == 0
                want = dict(kernel='wrnn_tile_kernel', units_per_wg=16, clusters=0, depth=0, rounds=1, slab_steps=T, workspace_bytes=auto['workspace_bytes'])
                for c in (0, 1):
                    assert debug_plan(L, tr, n, T, algo=TILE, clusters=c, noise_lib=noise_lib) == (0, want), (n_cus, n, T, c)


@pytest.mark.parametrize('W', WIDTHS)
def test_a_width_plans_the_wide_kernel(L, W):
    tr = dict(GENERIC, n_cus=256)
    for n in (1, 16, 17, 256 // W * 16):
        for T in (64, 2000):
            rc, pl = debug_plan(L, tr, n, T, algo=TILE, clusters=W)
            assert rc == 0, pl
            ws = pl.pop('workspace_bytes')
            assert pl == dict(kernel=WIDE, units_per_wg=16, clusters=W, depth=0, rounds=1, slab_steps=T), (n, T, pl)
            # tile's workspace plus the hand-off buffers: larger, by the tile count and the dims, not by T
            narrow = debug_plan(L, tr, n, T, algo=TILE)[1]['workspace_bytes']
            assert ws > narrow
            assert ws - narrow == debug_plan(L, tr, n, 7, algo=TILE, clusters=W)[1]['workspace_bytes'] - debug_plan(L, tr, n, 7, algo=TILE)[1]['workspace_bytes']
            tiles = (n + 15) // 16
            assert ws - narrow >= tiles * 5 * 256 * 16 * 4        # five stage vectors of rnn = fc = 256 rows x 16 segments per tile
    # ... and with the library's noise, whose T rows are the only part that grows with T
    a, b = (debug_plan(L, tr, 17, T, algo=TILE, clusters=W, noise_lib=1)[1]['workspace_bytes'] - debug_plan(L, tr, 17, T, algo=TILE, noise_lib=1)[1]['workspace_bytes']
            for T in (64, 2000))
    assert a == b > 0


@pytest.mark.parametrize('bad', [3, 16, -1, 5, 6, 7, 9, 64])
def test_any_other_width_is_refused_with_the_legal_ones(L, bad):
    rc, msg = debug_plan(L, dict(GENERIC, n_cus=256), 16, 100, algo=TILE, clusters=bad)
    assert rc == ERR_ARG and f'clusters = {bad}' in msg and '2, 4, 8' in msg and '0 or 1' in msg, msg


@pytest.mark.parametrize('n_cus', [64, 256])
@pytest.mark.parametrize('W', WIDTHS)
def test_one_round_at_most_one_workgroup_per_cu(L, n_cus, W):
    tr = dict(GENERIC, n_cus=n_cus)
    most = n_cus // W * 16                                  # ceil(n / 16) * W <= n_cus
    rc, pl = debug_plan(L, tr, most, 100, algo=TILE, clusters=W)
    assert rc == 0 and pl['kernel'] == WIDE, pl
    rc, msg = debug_plan(L, tr, most + 1, 100, algo=TILE, clusters=W)
    assert rc == ERR_ARG and WIDE in msg and f'at most {most} segments' in msg and 'plain algo tile' in msg, msg
    assert debug_plan(L, tr, most + 1, 100, algo=TILE)[1]['kernel'] == 'wrnn_tile_kernel'


@pytest.mark.parametrize('algo, name', [(12, 'tile_sparse'), (13, 'tile_bf16')])
def test_the_sparse_and_bf16_tile_kernels_have_no_wide_form(L, algo, name):
    tr = dict(GENERIC, n_cus=256, sp_nbp=1)
    assert debug_plan(L, tr, 16, 100, algo=algo)[0] == 0
    assert debug_plan(L, tr, 16, 100, algo=algo, clusters=1) == debug_plan(L, tr, 16, 100, algo=algo)
    for W in WIDTHS + (3,):
        rc, msg = debug_plan(L, tr, 16, 100, algo=algo, clusters=W)
        assert rc == ERR_ARG and 'only the float32 tile kernel' in msg and name in msg, msg


@pytest.mark.parametrize('W', WIDTHS)
def test_every_refusal_of_tile_keeps_its_text_under_the_new_name(L, W):
    def same(traits, **opts):
        rc, msg = debug_plan(L, traits, 16, 100, algo=TILE, **opts)
        rc_w, msg_w = debug_plan(L, traits, 16, 100, algo=TILE, clusters=W, **opts)
        assert rc == rc_w == ERR_ARG, (msg, msg_w)
        assert msg_w == msg.replace('wrnn_tile_kernel', WIDE), (msg, msg_w)
        return msg_w
    for name in SHIPPED:
        assert 'generic packs only' in same(dict(SHIPPED[name], n_cus=256))
    assert f'{tile_lds_bytes(2048, 2048, 80, 32)} bytes of LDS' in same(dict(GENERIC, n_cus=256, gH=2048, gF=2048))
    assert '<= 2048 classes' in same(dict(GENERIC, n_cus=256, mode=0, C=4096))
    assert 'partial step range' in same(dict(GENERIC, n_cus=256), t_begin=10, t_end=60)
    assert f'this call runs on {WIDE}' in same(dict(GENERIC, n_cus=256), sparse_groups=2)


def test_auto_never_answers_with_the_new_kernel(L):
    for n_cus in (32, 64, 256):
        for traits in [dict(GENERIC, n_cus=n_cus)] + [dict(SHIPPED[k], n_cus=n_cus) for k in SHIPPED]:
            for c in (0, 1, 2, 4, 8):
                for n in (1, 16, 64):
                    rc, pl = debug_plan(L, traits, n, 100, algo=0, clusters=c)
                    assert rc == 0 and pl['kernel'] != WIDE and not pl['kernel'].startswith('wrnn_tile'), (traits, c, n, pl)


def test_the_structs_and_the_abi_version_are_unchanged(L):
    from wavernn_amd import _lib
    assert ctypes.sizeof(_lib.Options) == 152 and _lib.Options.clusters.offset == 12     # sizeof(wrnn_options) of ABI 9; the field the width rides in
    assert ctypes.sizeof(_lib.PlanTraits) == 48
    assert L.wrnn_abi_version() == 9
    assert 'tile_wide' not in _lib.ALGOS and sorted(_lib.ALGOS.values()) == sorted(set(_lib.ALGOS.values()))
    assert 14 not in _lib.ALGOS.values()
    assert debug_plan(L, dict(GENERIC, n_cus=256), 16, 100, algo=14) == (ERR_ARG, 'unknown algo 14')


def test_header_with_the_new_comments_is_plain_c(tmp_path):
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'use_header.c'
    src.write_text('#include "wavernn_amd.h"\n'
                   'int probe(void) { wrnn_options o; wrnn_run_info i; o.clusters = 4; o.algo = WRNN_ALGO_TILE; i.clusters = o.clusters; return i.clusters + WRNN_ABI_VERSION; }\n'
                   'typedef char abi_is_nine[WRNN_ABI_VERSION == 9 ? 1 : -1];\n'
                   'typedef char options_keep_their_size[sizeof(wrnn_options) == 152 ? 1 : -1];\n'
                   'typedef char traits_keep_their_size[sizeof(wrnn_plan_traits) == 48 ? 1 : -1];\n')
    res = subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'), str(src)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    assert 'wrnn_tile_wide_kernel' in open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()


def test_the_engine_applies_its_tile_width_and_falls_back_with_one_warning(L):
    """`LoopEngine.tile_width` (what `WaveRNN.tile_width` sets) is the width of an algo='tile' call that names none; a call with more segments than the width
    takes runs on plain tile, and says so once.  The engine's own logic, on the planner of a 256-CU device (no pack, no device)."""
    import warnings
    from wavernn_amd import _lib
    from wavernn_amd.engine import LoopEngine

    class PlannerOnly:
        def wrnn_plan_segments(self, pack, n, T, o, i):
            ws = ctypes.c_size_t(0)
            t = _lib.PlanTraits(**dict(GENERIC, n_cus=256))
            return L.wrnn_debug_plan(ctypes.byref(t), n, T, 700, o, i, ctypes.byref(ws))
        wrnn_last_error = staticmethod(L.wrnn_last_error)

    eng = LoopEngine.__new__(LoopEngine)
    eng._timer = None                   # (nothing to release: no timer, no pack)
    eng.lib, eng._pack, eng._auto_floor, eng._tile_narrow, eng._tile_warned, eng.tile_width = PlannerOnly(), None, None, False, False, 8
    assert eng._tile_clusters('tile', 0, 512, 64) == 8
    assert eng._tile_clusters('tile', 2, 512, 64) == 2 and eng._tile_clusters('auto', 0, 16, 64) == 0 and eng._tile_clusters('tile_bf16', 0, 16, 64) == 0
    assert eng.plan(16, 64, algo='tile') == dict(kernel=WIDE, units_per_wg=16, clusters=8, depth=0, rounds=1, slab_steps=64)
    with pytest.warns(UserWarning, match='at most 512 segments'):
        assert eng._tile_clusters('tile', 0, 513, 64) == 0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert eng.plan(513, 64, algo='tile')['kernel'] == 'wrnn_tile_kernel'           # (said once)
    eng._tile_narrow = True                                                                # after a refused cooperative launch
    assert eng._tile_clusters('tile', 0, 16, 64) == 0
    eng.tile_width, eng._tile_narrow = 0, False
    assert eng.plan(16, 64, algo='tile')['kernel'] == 'wrnn_tile_kernel'
