"""The host side of LIVE streaming from the one-launch loop kernels (`wrnn_generate_segments_watched`, `generate_unbatched(live=True)`), without a GPU:
the two entry points in header, binding and library; the refusals of a watched call and its word count through the planner (`wrnn_debug_watch` on
hand-written traits); the pure function that decides which slices an observed progress value releases, under adversarial observation sequences; the
`loop_fn` stand-in path, which `live` must not change; and a discrete-event MODEL of the kernels' publish step (csrc/wrnn_device.h, publish_progress):

    every wave stores its samples of step t | end-of-step barrier | on a publishing step: every wave DRAINS its stores | BARRIER | one lane: RELEASE
    (write the L2 back) | WAIT for the write-back | store the word = t + 1

with an observer that reads the word and then the data at arbitrary times.  The built order never shows an unfinished step; each shortcut does."""
import ctypes
import heapq
import os
import random
import re

import numpy as np
import pytest
import torch

from test_planner_table import ERR_ARG, L      # noqa: F401  (L: the library fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ('wrnn_generic_kernel', 'wrnn_tile_kernel', 'wrnn_tile_sparse_kernel', 'wrnn_tile_bf16_kernel', 'wrnn_tile_wide_kernel')
TILE, TILE_SPARSE, TILE_BF16 = 10, 12, 13
#: a 256 / 256 MoL pack of non-shipped dims on a 256-CU device (tests/test_tile_plan.py), with a tile-sparse view; and two packs of the shipped dims
GENERIC = dict(n_cus=256, mode=1, C=30, generic=1, gH=256, gF=256, gM=80, gA=32, sp_max_blocks=256, sp_nbp=1, sp_fc=1)
SHIPPED = dict(dense_mol=dict(n_cus=256, mode=1, C=30, sp_max_blocks=512), raw512=dict(n_cus=256, mode=0, C=512, sp_max_blocks=512),
               small_device=dict(n_cus=32, mode=1, C=30, sp_max_blocks=512))


def watch(L, traits, n, T, progress=None, words=0, every=1, **opts):
    """wrnn_debug_watch -> (rc, word count or the error text)"""
    from wavernn_amd import _lib
    t, o, w = _lib.PlanTraits(**traits), _lib.Options(**opts), ctypes.c_int32(-1)
    rc = L.wrnn_debug_watch(ctypes.byref(t), n, T, ctypes.byref(o), -1 if progress is None else int(progress), words, every, ctypes.byref(w))
    return rc, (int(w.value) if rc == 0 else L.wrnn_last_error().decode())


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_both_entry_points_are_declared_bound_and_exported(L):
    from wavernn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'wavernn_amd.h')).read()
    for name in ('wrnn_generate_segments_watched', 'wrnn_watch_words', 'wrnn_debug_watch'):
        assert re.search(r'\bint ' + name + r'\(', header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # appended: behind everything the header declared before
    assert header.index('int wrnn_generate_segments_watched(') > header.index('int wrnn_debug_taco_group_of(')
    assert re.search(r'unsigned \*progress, int32_t progress_words, int32_t progress_every\);', header)
    assert L.wrnn_abi_version() == 9 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.Options) == 152
    assert len(L.wrnn_generate_segments_watched.argtypes) == len(L.wrnn_generate_segments.argtypes) + 3


def test_engine_names_the_five_kernels():
    from wavernn_amd import engine
    assert tuple(engine.WATCHABLE_KERNELS) == FIVE
    assert not set(engine.WATCHABLE_KERNELS) & set(engine.RESUMABLE_KERNELS)


# ---- the planner's answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SHIPPED))
def test_shipped_dims_are_refused_and_the_message_names_the_five_kernels(L, name):
    for progress in (None, True):
        rc, msg = watch(L, SHIPPED[name], 16, 2000, progress=progress, words=64, every=16)
        assert rc == ERR_ARG, msg
        assert all(k in msg for k in FIVE), msg
        assert 't_begin / t_end' in msg and 'plans onto wrnn_' in msg, msg
    # ... also when a kernel that continues a call is asked for by name
    rc, msg = watch(L, SHIPPED['dense_mol'], 16, 2000, algo=7)
    assert rc == ERR_ARG and 'plans onto wrnn_chain_kernel' in msg, msg


@pytest.mark.parametrize('n', [1, 16, 17, 64])
def test_one_word_per_workgroup_that_writes_out(L, n):
    tiles = (n + 15) // 16
    assert watch(L, GENERIC, n, 2000) == (0, n)                              # wrnn_generic_kernel: one workgroup per segment
    for algo in (TILE, TILE_SPARSE, TILE_BF16):
        assert watch(L, GENERIC, n, 2000, algo=algo) == (0, tiles), algo        # one workgroup per tile of 16 segments
    for width in (2, 4, 8):
        assert watch(L, GENERIC, n, 2000, algo=TILE, clusters=width) == (0, tiles), width      # member 0 of every tile
    # the whole call's answers: with a progress buffer that is just large enough
    assert watch(L, GENERIC, n, 2000, progress=True, words=n, every=16) == (0, n)
    assert watch(L, GENERIC, n, 2000, progress=True, words=tiles, every=64, algo=TILE, clusters=4) == (0, tiles)


def test_each_refusal_names_its_cause(L):
    rc, msg = watch(L, GENERIC, 17, 2000, progress=True, words=2, every=0, algo=TILE)
    assert rc == ERR_ARG and 'progress_every = 0' in msg and 'wrnn_tile_kernel' in msg, msg
    rc, msg = watch(L, GENERIC, 17, 2000, progress=True, words=2, every=-3, algo=TILE)
    assert rc == ERR_ARG and 'progress_every = -3' in msg, msg
    rc, msg = watch(L, GENERIC, 17, 2000, progress=True, words=1, every=16, algo=TILE)
    assert rc == ERR_ARG and 'progress_words = 1' in msg and ' 2 for 17 segments' in msg and 'wrnn_tile_kernel' in msg, msg
    rc, msg = watch(L, GENERIC, 17, 2000, progress=True, words=16, every=16)
    assert rc == ERR_ARG and 'progress_words = 16' in msg and ' 17 for 17 segments' in msg and 'wrnn_generic_kernel' in msg, msg
    rc, msg = watch(L, GENERIC, 17, 2000, progress=False, words=17, every=16)
    assert rc == ERR_ARG and 'NULL' in msg and 'wrnn_generic_kernel' in msg, msg
    for kw in (dict(t_begin=0, t_end=1000), dict(t_begin=1000, t_end=2000), dict(t_begin=16, t_end=32)):
        for progress in (None, True):
            rc, msg = watch(L, GENERIC, 17, 2000, progress=progress, words=17, every=16, algo=TILE, clusters=2, **kw)
            assert rc == ERR_ARG and 'partial' in msg and f"[{kw['t_begin']}, {kw['t_end']})" in msg and 'wrnn_tile_wide_kernel' in msg, msg
    assert watch(L, GENERIC, 17, 2000, progress=True, words=17, every=16, t_begin=0, t_end=2000) == (0, 17)      # the whole range, spelt out
    # what the planner refuses for a plain call stays refused, in its own words
    rc, msg = watch(L, GENERIC, 17, 2000, algo=TILE, clusters=3)
    assert rc == ERR_ARG and 'wrnn_options.clusters = 3' in msg, msg
    rc, msg = watch(L, dict(GENERIC, sp_nbp=0), 17, 2000, algo=TILE_SPARSE)
    assert rc == ERR_ARG and 'no tile-sparse view' in msg, msg


def test_the_typed_wrapper(L):
    from wavernn_amd import _lib
    assert _lib.watch_words_host(_lib.PlanTraits(**GENERIC), 33, 500, _lib.Options(algo=TILE)) == 3
    with pytest.raises(_lib.WrnnError, match='progress_every = 0'):
        _lib.watch_words_host(_lib.PlanTraits(**GENERIC), 33, 500, None, progress=True, progress_words=33, progress_every=0)


# ---- which slices does an observed m release ---------------------------------------------------------------------------------
def _slices(T, k):
    return [(a, min(T, a + k)) for a in range(0, T, k)]


def _drive(slices, T, observations):
    """feed the observations; returns the release log [(index, m at release)]"""
    from wavernn_amd.batch import live_release
    done, log = 0, []
    for m in observations:
        upto = live_release(slices, done, m)
        assert done <= upto <= len(slices)
        log += [(i, m) for i in range(done, upto)]
        done = upto
    return log


@pytest.mark.parametrize('T, k', [(3712, 997), (2944, 997), (2000, 2000), (2000, 1), (5, 64), (4096, 1024)])
def test_slices_are_released_once_in_order_and_never_early(T, k):
    slices = _slices(T, k)
    rng = random.Random(T * 31 + k)
    sequences = {
        'stuck at 0, then T': [0] * 50 + [T],
        'straight to T': [T],
        'multiples of 16, repeated': [m for m in range(0, T, 16) for _ in range(3)] + [T],
        'no multiple of the chunk': list(range(0, T, 7)) + [T],
        'one step at a time': list(range(0, min(T, 300))) + [T, T, T],
        'random, non-decreasing, repeated': sorted(rng.randrange(T + 1) for _ in range(200)) + [T],
        'running backwards in between': [rng.randrange(T + 1) for _ in range(200)] + [T],
    }
    for name, obs in sequences.items():
        log = _drive(slices, T, obs)
        assert [i for i, _ in log] == list(range(len(slices))), name                 # every slice exactly once, in order, all of them once m = T
        assert all(slices[i][1] <= m for i, m in log), name                          # never before m covers it
    assert _drive(slices, T, [0] * 100) == []                                        # a kernel that never gets anywhere releases nothing
    first = _drive(slices, T, [slices[0][1] - 1, slices[0][1]])
    assert first and first[0] == (0, slices[0][1]) and all(m == slices[0][1] for _, m in first)


# ---- the stand-in path: `live` changes nothing there ---------------------------------------------------------------------------
def test_live_changes_nothing_under_loop_fn():
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import SHIPPED as HP, random_mel, random_state_dict
    sd = random_state_dict(61, mode='MOL')
    model = WaveRNN(**HP, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    mels, seeds = [random_mel(710 + k, f) for k, f in enumerate([22, 24, 21])], [41, 42, 43]

    def loop_fn(mels_up, aux, seg_pos, seg_lim, T, noise, hop):            # any deterministic stand-in will do: the chunking is under test, not the loop
        g = torch.Generator().manual_seed(int(np.asarray(seg_pos).sum()) + T)
        return torch.rand(len(seg_pos), T, generator=g) * 2 - 1

    runs = {}
    for live in (False, True):
        calls = []
        outs = generate_unbatched(model, mels, False, seeds, noise_source='library', chunk_steps=997, loop_fn=loop_fn, live=live,
                                  on_chunk=lambda u, start, s: calls.append((u, start, s)))
        runs[live] = (outs, calls)
    (a, ca), (b, cb) = runs[False], runs[True]
    assert len(ca) > 3 * 5 and [(u, s) for u, s, _ in ca] == [(u, s) for u, s, _ in cb]
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(ca, cb))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert sorted({s for _, s, _ in ca}) == list(range(0, 23 * 275, 997))


# ---- a discrete-event model of the publish step ------------------------------------------------------------------------------
class PublishSim:
    """One workgroup of `waves` waves; wave w stores its own samples of every step (keys (w, t)).  A store is in flight for a random time, then sits in
    the XCD's L2; only a write-back puts what the L2 holds at that moment into memory, which is all that the observer -- a copy or kernel launched
    later, anywhere -- can see.  The word goes to memory directly (an agent-scope atomic), after a delay of its own.  Barriers order the waves and
    nothing else: only a drain waits for a wave's stores, only the wait behind the release for the write-back."""

    def __init__(self, seed, waves=4, steps=24, every=4, drain=True, barrier=True, wait_release=True, flag_after_release=True):
        self.rng = random.Random(seed)
        self.waves, self.steps, self.every = waves, steps, every
        self.drain, self.barrier, self.wait_release, self.flag_after_release = drain, barrier, wait_release, flag_after_release
        self.l2, self.mem, self.word = set(), set(), 0
        self.events, self.seq, self.now = [], 0, 0.0
        self.violations, self.seen = [], []

    def delay(self, scale=1.0):
        d = self.rng.expovariate(1.0 / scale)
        if self.rng.random() < 0.05:
            d += 20.0 * self.rng.random()                # now and then: later than many whole steps (a step's work is ~1)
        return d

    def at(self, when, fn):
        self.seq += 1
        heapq.heappush(self.events, (when, self.seq, fn))

    def program(self, w):
        for t in range(self.steps):
            yield ('work', self.rng.random() * self.rng.choice((0.2, 1.0, 3.0)))
            yield ('store', (w, t))
            yield ('bar',)                               # the last barrier of step t
            done = t + 1
            if done % self.every == 0 or done == self.steps:
                if not self.flag_after_release and w == 0:
                    yield ('flag', done)                 # the shortcut: the word first, the ordering afterwards
                if self.drain:
                    yield ('drain',)
                if self.barrier:
                    yield ('bar',)
                if w == 0:
                    yield ('release',)
                    if self.wait_release:
                        yield ('wait_release',)
                    if self.flag_after_release:
                        yield ('flag', done)

    def run(self):
        pending = [0] * self.waves
        waiting, at_bar = {}, []
        writebacks = [0]
        last_flag = [0.0]
        procs = [self.program(w) for w in range(self.waves)]
        finished = [0]

        def wake():
            for w, cond in list(waiting.items()):
                if cond():
                    del waiting[w]
                    resume(w)

        def resume(w):
            while True:
                try:
                    cmd = next(procs[w])
                except StopIteration:
                    finished[0] += 1
                    return
                if cmd[0] == 'work':
                    self.at(self.now + cmd[1], lambda w=w: resume(w))
                    return
                if cmd[0] == 'store':
                    pending[w] += 1

                    def land(key=cmd[1], w=w):
                        self.l2.add(key)
                        pending[w] -= 1
                        wake()
                    self.at(self.now + self.delay(), land)
                elif cmd[0] == 'bar':
                    at_bar.append(w)
                    if len(at_bar) < self.waves:
                        return
                    others = [x for x in at_bar if x != w]
                    del at_bar[:]
                    for x in others:
                        self.at(self.now, lambda x=x: resume(x))
                elif cmd[0] == 'drain':
                    if pending[w]:
                        waiting[w] = lambda w=w: pending[w] == 0
                        return
                elif cmd[0] == 'release':
                    writebacks[0] += 1
                    snapshot = set(self.l2)

                    def written(snapshot=snapshot):
                        self.mem |= snapshot
                        writebacks[0] -= 1
                        wake()
                    self.at(self.now + self.delay(2.0), written)
                elif cmd[0] == 'wait_release':
                    if writebacks[0]:
                        waiting[w] = lambda: writebacks[0] == 0
                        return
                elif cmd[0] == 'flag':
                    when = max(self.now + self.delay(0.3), last_flag[0] + 1e-6)      # one address: its stores land in order
                    last_flag[0] = when

                    def land(v=cmd[1]):
                        self.word = v
                    self.at(when, land)

        def observe():
            m = self.word                                # the look ...

            def read(m=m):                               # ... and, launched after it, whatever reads out[:, :m]
                self.seen.append(m)
                missing = [(w, t) for t in range(m) for w in range(self.waves) if (w, t) not in self.mem]
                if missing:
                    self.violations.append(f'word = {m} but {len(missing)} samples of steps < {m} are not in memory, e.g. {missing[0]}')
            self.at(self.now + self.rng.random() * self.rng.choice((0.0, 0.1, 3.0)), read)

        for w in range(self.waves):
            resume(w)
        horizon = 3.0 * self.steps
        for _ in range(12 * self.steps):
            self.at(self.rng.random() * horizon, observe)
        while self.events:
            self.now, _, fn = heapq.heappop(self.events)
            fn()
        if finished[0] != self.waves:
            self.violations.append(f'{self.waves - finished[0]} waves wait forever')
        elif self.word != self.steps:
            self.violations.append(f'the last word is {self.word}, not {self.steps}')
        return self.violations


SEEDS = range(40)
SHAPES = [(waves, every) for waves in (1, 4, 8) for every in (1, 4, 16)]


@pytest.mark.parametrize('waves, every', SHAPES)
def test_the_built_order_never_shows_an_unfinished_step(waves, every):
    between = 0
    for seed in SEEDS:
        sim = PublishSim(seed, waves, 24, every)
        assert sim.run() == [], (waves, every, seed)
        assert all(m % every == 0 or m == 24 for m in sim.seen), sim.seen
        between += sum(0 < m < 24 for m in sim.seen)
    assert between > 0                                   # (the observer did look while the kernel ran: the model is not vacuous)


def broken(**kw):
    return sum(bool(PublishSim(seed, waves, 24, every, **kw).run()) for seed in SEEDS for waves, every in SHAPES if waves > 1 or 'barrier' not in kw)


def test_a_word_stored_before_the_drain_is_detected():
    assert broken(drain=False) > 0


def test_a_publish_without_the_barrier_is_detected():
    """One lane releases and signals for stores of OTHER waves that it never waited for."""
    assert broken(barrier=False) > 0


def test_a_word_by_a_lane_that_did_not_wait_is_detected():
    """The word leaves while the write-back of the release is still under way -- or before the release was even issued."""
    assert broken(wait_release=False) > 0
    assert broken(flag_after_release=False) > 0
