"""CPU tests of the library's own sampling noise (wrnn_options.noise_lib, csrc/wrnn_philox.h, csrc/wrnn_noise.hip) through `wrnn_noise_fill_host`
and `wrnn_debug_plan`: no HIP device is needed.  The generator is restated here in numpy; the values the library writes must be that restatement's
-- MOL bit for bit, RAW within two logf implementations."""
import ctypes

import numpy as np
import pytest

from test_planner_table import ERR_ARG, L, debug_plan      # noqa: F401  (L: the library fixture)

MOL, RAW = 1, 0
ALGO = dict(auto=0, stream=1, sparse=5, duo=6, chain=7)
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k):
    """Philox4x32-10 (Random123 constants) on uint64 arrays holding 32-bit words: c = 4 counter words, k = 2 key words -> 4 output words."""
    c = [np.asarray(x, np.uint64) & U32 for x in c]
    k = [np.asarray(x, np.uint64) & U32 for x in k]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & U32, (k[1] + np.uint64(0xBB67AE85)) & U32]
    return c


def words(seed, ids, t0, t1, J):
    """[t1 - t0, B, J] uint64: the 32-bit word of (step, segment, index j) = word j % 4 of block (t, j / 4, id lo, id hi) under key (seed lo, hi)."""
    ids = np.asarray(ids, np.uint64)
    t, b, q = np.meshgrid(np.arange(t0, t1, dtype=np.uint64), ids, np.arange((J + 3) // 4, dtype=np.uint64), indexing='ij')
    blk = philox4x32_10([t, q, b & U32, b >> np.uint64(32)], [np.uint64(seed) & U32, np.uint64(seed) >> np.uint64(32)])
    return np.stack(blk, axis=-1).reshape(t1 - t0, len(ids), -1)[:, :, :J]


def mol_values(w):
    """u = min(((w >> 8) * 2^-24) * 0.99998f + 1e-5f, 0.99999f), every operation rounded to float32."""
    f = np.float32
    k = (w >> np.uint64(8)).astype(np.float32)
    u = (k * f(2.0 ** -24)) * f(0.99998) + f(1e-5)
    assert u.dtype == np.float32
    return np.minimum(u, f(0.99999))


def mol_layout(v):
    """[T, B, 11] -> [T, 11 B]: 10 B mixture uniforms (segment-major), then B logistic uniforms."""
    T, B, _ = v.shape
    return np.concatenate([v[:, :, :10].reshape(T, 10 * B), v[:, :, 10]], axis=1)


def raw_reference(w):
    """-log in float64 of the float32 argument min(((w >> 8) + 0.5f) * 2^-24, 1 - 2^-24)."""
    f = np.float32
    x = np.minimum(((w >> np.uint64(8)).astype(np.float32) + f(0.5)) * f(2.0 ** -24), f(1.0 - 2.0 ** -24))
    assert x.dtype == np.float32
    return -np.log(x.astype(np.float64))


def fill(mode, B, C, t0, t1, seed, ids=None):
    from wavernn_amd import _lib
    return _lib.noise_fill_host('MOL' if mode == MOL else 'RAW', B, C, t0, t1, seed, ids)


IDS = np.array([7, (0xDEADBEEF << 32) | 3, 2 ** 64 - 1], np.uint64)
SEED = 0x0123456789ABCDEF


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32_10 (recalled from its kat_vectors file, not re-read)."""
    assert [int(x) for x in philox4x32_10([0, 0, 0, 0], [0, 0])] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 0xFFFFFFFF
    assert [int(x) for x in philox4x32_10([ones] * 4, [ones] * 2)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_value_formulas_at_the_edges():
    """The extreme 24-bit words: MoL stays inside [1e-5, 1 - 1e-5] (the largest word lands an ulp below the top: the clamp is a guard), RAW stays finite
    and > 0 (its clamp is needed: without it the last word's argument rounds to 1 and the variate to 0, which the sampler divides by)."""
    f = np.float32
    w = np.array([0, 1 << 8, (2 ** 23) << 8, (2 ** 24 - 2) << 8, 2 ** 32 - 1], np.uint64)
    u = mol_values(w)
    assert u[0] == f(1e-5) and f(0.99999) - u[-1] <= f(2.0 ** -23) and np.all((u >= f(1e-5)) & (u <= f(0.99999))) and np.all(np.diff(u) > 0)
    assert f(2 ** 24 - 1) + f(0.5) == f(2 ** 24)
    q = raw_reference(w)
    assert np.all(np.isfinite(q)) and np.all(q > 0) and q[-1] == -np.log(1.0 - 2.0 ** -24)


@pytest.mark.parametrize('ids', [None, IDS])
def test_mol_is_the_restatement_bit_for_bit(L, ids):
    B = 3
    got = fill(MOL, B, 30, 0, 5, SEED, ids)
    want = mol_layout(mol_values(words(SEED, np.arange(B) if ids is None else ids, 0, 5, 11)))
    assert got.shape == (5, 11 * B) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.min() >= np.float32(1e-5) and got.max() <= np.float32(1.0 - 1e-5)
    # key 0, segment id 0, step 0, indices 0..3: the all-zero counter and key of the known-answer test
    z = fill(MOL, 1, 30, 0, 1, 0)
    assert np.array_equal(z[0, :4], mol_values(np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], np.uint64)))


@pytest.mark.parametrize('C', [512, 7])
@pytest.mark.parametrize('ids', [None, IDS])
def test_raw_is_minus_log_of_the_restated_word(L, C, ids):
    B = 3
    got = fill(RAW, B, C, 0, 5, SEED, ids)
    want = raw_reference(words(SEED, np.arange(B) if ids is None else ids, 0, 5, C))
    assert got.shape == (5, B, C) and got.dtype == np.float32
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    # two logf implementations, each within an ulp or so of -log: a few float32 ulps (6e-8 each) is the margin
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize('mode,C', [(MOL, 30), (RAW, 512), (RAW, 7)])
def test_a_step_range_is_a_slice_and_ids_own_their_columns(L, mode, C):
    B = 3
    whole = fill(mode, B, C, 0, 5, SEED, IDS)
    assert np.array_equal(fill(mode, B, C, 2, 5, SEED, IDS), whole[2:5])
    perm = np.array([2, 0, 1])
    moved = fill(mode, B, C, 0, 5, SEED, IDS[perm])
    if mode == MOL:
        mix, logi = whole[:, :10 * B].reshape(5, B, 10), whole[:, 10 * B:]
        assert np.array_equal(moved, np.concatenate([mix[:, perm].reshape(5, 10 * B), logi[:, perm]], axis=1))
    else:
        assert np.array_equal(moved, whole[:, perm])
    # another seed, another id: other values; the default ids are 0 .. B - 1
    assert not np.array_equal(fill(mode, B, C, 0, 5, SEED + 1, IDS), whole)
    assert np.array_equal(fill(mode, B, C, 0, 5, SEED), fill(mode, B, C, 0, 5, SEED, np.arange(B, dtype=np.uint64)))


def test_fill_argument_errors(L):
    out = np.zeros(64, np.float32)
    for args, needle in (((2, 1, 30, 0, 1), b'unknown mode'), ((MOL, 0, 30, 0, 1), b'bad noise shape'), ((MOL, 1, 30, 3, 3), b'bad noise shape'),
                         ((RAW, 1, 0, 0, 1), b'bad noise shape'), ((MOL, 1, 30, -1, 1), b'bad noise shape')):
        assert L.wrnn_noise_fill_host(*args, 0, None, out.ctypes.data) == ERR_ARG
        assert needle in L.wrnn_last_error(), L.wrnn_last_error()
    assert L.wrnn_noise_fill_host(MOL, 1, 30, 0, 1, 0, None, None) == ERR_ARG


# ---- the planner: wrnn_options.noise_lib adds one slab of noise to the workspace and nothing else ---------------------------------------------
DENSE_MOL = dict(n_cus=256, mode=MOL, C=30, sp_max_blocks=512)
DENSE_RAW = dict(n_cus=256, mode=RAW, C=512, sp_max_blocks=512)
SPARSE_MOL = dict(n_cus=256, mode=MOL, C=30, sp_nbp=48, sp_max_blocks=40, sp_fc=1)
SPARSE_RAW = dict(n_cus=256, mode=RAW, C=512, sp_nbp=48, sp_max_blocks=40, sp_fc=1)
ROWS = [('chain', 'wrnn_chain_kernel', DENSE_MOL, DENSE_RAW, 19), ('duo', 'wrnn_duo_kernel', DENSE_MOL, DENSE_RAW, 300),
        ('sparse', 'wrnn_sparse_kernel', SPARSE_MOL, SPARSE_RAW, 300), ('stream', 'wrnn_stream_kernel', DENSE_MOL, DENSE_RAW, 19)]


def al256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize('algo,kernel,mol,raw,n', ROWS)
@pytest.mark.parametrize('slab_steps', [0, 37])
def test_workspace_grows_by_one_slab_of_noise(L, algo, kernel, mol, raw, n, slab_steps):
    T = 1210
    for tr in (mol, raw):
        per_step = n * (11 if tr['mode'] == MOL else tr['C']) * 4
        rc0, without = debug_plan(L, tr, n, T, algo=ALGO[algo], slab_steps=slab_steps)
        rc1, with_ = debug_plan(L, tr, n, T, algo=ALGO[algo], slab_steps=slab_steps, noise_lib=1)
        assert rc0 == 0 and rc1 == 0, (without, with_)
        assert with_['kernel'] == without['kernel'] == kernel
        steps = T if algo == 'stream' else with_['slab_steps']
        assert with_['workspace_bytes'] - without['workspace_bytes'] == al256(steps * per_step), (tr, without, with_)
        # the split is the same; the slab too, except where a RAW slab is now what holds 2 GB of noise
        for key in ('units_per_wg', 'clusters', 'depth', 'rounds'):
            assert with_[key] == without[key]
        assert with_['slab_steps'] <= without['slab_steps'] and (with_['slab_steps'] == without['slab_steps'] or tr['mode'] == RAW)
        assert steps * per_step <= 2 << 30


def test_a_raw_slab_holds_two_gigabytes_of_noise_at_most(L):
    for n, slab in ((256, 4096), (300, 3495), (4096, 256)):
        rc, pl = debug_plan(L, DENSE_RAW, n, 12100, algo=ALGO['duo'], noise_lib=1)
        assert rc == 0 and pl['slab_steps'] == slab == min(4096, (2 << 30) // (n * 512 * 4)), (n, pl)
        assert debug_plan(L, DENSE_RAW, n, 12100, algo=ALGO['duo'])[1]['slab_steps'] == 4096


def test_generic_dims_take_the_whole_call_of_noise(L):
    tr = dict(n_cus=256, mode=RAW, C=64, generic=1, gH=256, gF=256, gM=80, gA=32)
    a, b = debug_plan(L, tr, 5, 300)[1], debug_plan(L, tr, 5, 300, noise_lib=1)[1]
    assert a['kernel'] == b['kernel'] == 'wrnn_generic_kernel' and b['workspace_bytes'] - a['workspace_bytes'] == al256(300 * 5 * 64 * 4)


def test_without_the_option_every_answer_is_what_it_was(L):
    """noise_lib = 0, and a caller whose struct ends in front of the fields (whatever lies behind it is not read): plan and size as if the fields did not exist."""
    from wavernn_amd import _lib
    old_size = _lib.Options.noise_lib.offset
    assert old_size == _lib.Options.sparse_groups.offset + 4 and ctypes.sizeof(_lib.Options) == old_size + 4 + 8 + 8
    for algo, kernel, mol, raw, n in ROWS:
        for tr in (mol, raw):
            base = debug_plan(L, tr, n, 1210, algo=ALGO[algo])
            assert base[0] == 0 and debug_plan(L, tr, n, 1210, algo=ALGO[algo], noise_lib=0, noise_seed=99, noise_seg_id=1 << 20) == base
            t, o, i, ws = _lib.PlanTraits(**tr), _lib.Options(algo=ALGO[algo], noise_lib=1, noise_seed=5), _lib.RunInfo(), ctypes.c_size_t(0)
            o.struct_bytes = old_size
            assert L.wrnn_debug_plan(ctypes.byref(t), n, 1210, 700, ctypes.byref(o), ctypes.byref(i), ctypes.byref(ws)) == 0
            assert (i.kernel.decode(), i.slab_steps, ws.value) == (base[1]['kernel'], base[1]['slab_steps'], base[1]['workspace_bytes'])


def test_option_argument_errors(L):
    rc, msg = debug_plan(L, DENSE_MOL, 19, 100, noise_lib=2)
    assert rc == ERR_ARG and 'noise_lib = 2' in msg
    rc, msg = debug_plan(L, DENSE_MOL, 19, 100, noise_lib=-1)
    assert rc == ERR_ARG and 'noise_lib = -1' in msg
    # noise_lib = 1 and a noise pointer: refused before anything else is looked at -- no caller may believe their tensor was used
    from wavernn_amd import _lib
    o = _lib.Options(noise_lib=1)
    noise = np.zeros(16, np.float32)
    rc = L.wrnn_generate_segments(None, 1, 10, None, None, 275, 275, 1, None, None, noise.ctypes.data, None, None, 0, ctypes.byref(o), None)
    assert rc == ERR_ARG and b'`noise` must be NULL' in L.wrnn_last_error()
    g = _lib.Geometry(1, 10, 0, 275, 275, 1)
    rc = L.wrnn_generate(None, ctypes.byref(g), None, None, noise.ctypes.data, None, None, 0, ctypes.byref(o), None)
    assert rc == ERR_ARG and b'`noise` must be NULL' in L.wrnn_last_error()
    # without the option a NULL `noise` stays the error it was
    o = _lib.Options()
    rc = L.wrnn_generate_segments(None, 1, 10, None, None, 275, 275, 1, None, None, None, None, None, 0, ctypes.byref(o), None)
    assert rc == ERR_ARG and L.wrnn_last_error() == b'NULL argument'


def test_corpus_stream_ids_do_not_depend_on_the_batch():
    """generate_corpus(noise_source='library') with a loop stand-in that hands back each segment's logistic uniforms: an utterance's noise is the same in
    a batch of three, alone, and in chunks -- (seeds[u] & 0xffffffff) << 32 | fold index, key model.noise_key."""
    import torch
    from wavernn_amd import _lib
    from wavernn_amd.batch import generate_corpus, library_seg_ids
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import SHIPPED, random_mel

    def loop_fn(mels_up, aux, seg_pos, seg_lim, T, noise, hop):
        n = len(seg_pos)
        assert noise.shape == (T, 11 * n)
        return noise[:, 10 * n:].T.contiguous()

    model = WaveRNN(**SHIPPED, mode='MOL')
    model.noise_key = 0xFEEDFACE12345678
    frames, seeds = (24, 22, 21), [71, 2 ** 32 + 5, 9]
    mels = [torch.from_numpy(random_mel(1700 + k, f)).unsqueeze(0) for k, f in enumerate(frames)]
    segs, plan = generate_corpus(model, mels, 550, 55, False, seeds, loop_fn=loop_fn, noise_source='library', return_segments=True)
    split, _ = generate_corpus(model, mels, 550, 55, False, seeds, loop_fn=loop_fn, noise_source='library', return_segments=True,
                               max_segments_per_launch=int(plan.folds.max()))
    assert np.array_equal(segs, split) and segs.shape == (int(plan.folds.sum()), 660)
    for u in range(3):
        alone, _ = generate_corpus(model, mels[u:u + 1], 550, 55, False, seeds[u:u + 1], loop_fn=loop_fn, noise_source='library', return_segments=True)
        f0, nf = int(plan.first[u]), int(plan.folds[u])
        assert np.array_equal(alone, segs[f0:f0 + nf])
        ids = library_seg_ids(seeds[u], nf)
        assert ids.dtype == np.uint64 and [int(i) for i in ids[:2]] == [(seeds[u] & 0xFFFFFFFF) << 32, ((seeds[u] & 0xFFFFFFFF) << 32) + 1]
        want = _lib.noise_fill_host('MOL', nf, 30, 0, 660, model.noise_key, ids)[:, 10 * nf:].T
        assert np.array_equal(alone.astype(np.float32), want)
    with pytest.raises(ValueError):
        generate_corpus(model, mels, 550, 55, False, None, loop_fn=loop_fn, noise_source='library')
