"""A discrete-event MODEL of wrnn_sparse_kernel's exchange with TWO groups of segments per cluster (wrnn_options.sparse_groups = 2; csrc/wrnn_sparse.hip,
`NS = 2`): the gathered-fc protocol of tests/test_sparse_exchange_model.py (SparseFcSim), run by every wave for slot 0 and then for slot 1, stage by stage:

    rnn1 half:  drain | barrier | for s: x_{t-1}[s] (tagged) -> cell -> publish x1[s], h1[s] | for s: gather h1[s] -> gh |
                for s: its fc tile (q = 0: gather x2[s] -> y1[s]; q = 1: gather y1[s] -> y2[s]), RE-ARM its words of entry t + 2 of slot s |
                for s: gather cI(t + 1)[s] -> W_ih . cI
    rnn2 half:  drain | barrier | for s: x_{t-1}[s], gather x1[s] -> cell -> publish x2[s], h2[s] | for s: its fc tile, RE-ARM |
                j = 0: for s: poll ALL of y2[s] -> barrier -> sample -> x_t[s] as a tagged word | for s: gather h2[s] -> gh | for s: form cI(t + 3)[s]

What the model settles:
  * every slot has its OWN region of the exchange buffer (all layers, its tagged x words included): group g of a round uses region g whichever
    cluster and slot runs it -- no per-slot offset inside a region, nothing of the one-group layout moves;
  * the x_t word a wave waits for is its slot's: a wave of slot 1 that looked at slot 0's word would take a value of the right step and the wrong group
    (`x_from=0` below);
  * the one-group skew arguments hold PER SLOT.  A slot's events keep, in every wave, the order and the waits they have in the one-group kernel; the
    other slot's stages in between are time that passes, which adversarial timing already allows for.  So "x_t[s] exists => everyone finished step
    t - 1 of slot s" (the sampler read ALL of y2[s](t); those waves passed the top of step t, which lies behind every stage of step t - 1 of BOTH
    slots), the ONE drain and ONE barrier at the top of a step cover both slots' re-arms and cI stores, and cI formed three steps ahead is drained
    before any reader of that slot can have seen x_{t+1}[s].  What does NOT carry over is anything ACROSS slots: slot 0's progress says nothing about
    slot 1's ring, hence the per-slot x word and the per-slot re-arm;
  * nothing waits in a circle: order the publications by (step, stage along the chain, slot); a wave waiting in stage k of slot s of step t waits only
    for publications that come earlier in that order, and has itself only waited for earlier ones -- the model's "everybody finishes";
  * a slot without a group in this round (<= 16 groups: every second slot; 17 .. 31: the last clusters') is skipped by every wave alike: nobody
    publishes there, so nobody may wait there (`wait_empty` below dead-locks).
Adversarial timing as in tests/test_duo_exchange_model.py (its engine: stores land after random delays, out of order, now and then later than ten whole
steps; only a drain waits for them).  A model of the protocol, not of the HIP code: tests/test_gpu_sparse_two_groups.py runs that."""
import heapq
import random

from test_duo_exchange_model import DuoSim, RING, SENT


class TwoGroupSim(DuoSim):
    """second: 'full' | 'ragged' (slot 1 has fewer live segments: its waves look at fewer words) | 'empty' (no group in slot 1 this round)."""

    def __init__(self, seed, n=2, steps=20, ahead=2, drain=True, barrier=True, cond_lead=2, density=0.5, second='full', x_from=1, wait_empty=False,
                 limit=60000.0):
        super().__init__(seed, n_wg=n, slots=1, steps=steps)            # (the engine only: clock, stores, pending counts; the memory is replaced below)
        self.n, self.ahead, self.drain, self.use_barrier, self.cond_lead = n, ahead, drain, barrier, cond_lead
        self.live = (True, second != 'empty')
        self.x_from, self.wait_empty, self.limit = x_from, wait_empty, limit
        ring = lambda producers, entries: [[[SENT] * producers for _ in range(entries)] for _ in range(2)]       # [slot][entry][producer]
        self.mem = {l: ring(2 * n, RING) for l in ('h1', 'x1', 'h2', 'x2', 'cI', 'y1', 'y2')}
        self.mem['xt'] = ring(1, 2)                                # words (step, slot of the sampler that wrote it)
        self.bar = {}
        pat = random.Random(1000 + seed)
        dens = (density, density * 0.5 if second == 'ragged' else density)
        self._sub = {}

        def subset(who, layer, s):
            key = (who, layer, s)
            if key not in self._sub:
                self._sub[key] = [k for k in range(2 * n) if pat.random() < dens[s]]
            return self._sub[key]
        self.subset = subset

    def resume(self, p):
        try:
            kind, arg = next(p)
        except StopIteration:
            self.done += 1
            return
        if kind == 'work':
            self.at(self.rng.choice([0.2, 1.0, 2.0, 6.0]) * arg, lambda: self.resume(p))
        elif kind == 'gather':                                   # the words of `idxs` (None: all) of slot s, entry t: re-read until none is the sentinel
            layer, s, t, idxs = arg

            def poll():
                words = self.mem[layer][s][t % RING]
                ks = range(len(words)) if idxs is None else idxs
                if any(words[k] is SENT for k in ks):
                    self.at(0.5, poll)
                    return
                for k in ks:
                    if words[k] != t:
                        self.violations.append(f'{layer}[slot {s}][{k}] read as step {words[k]} while gathering step {t}')
                self.resume(p)
            poll()
        elif kind == 'xtag':                                     # a wave of slot s waits for x_t: the tagged word of slot `src`
            s, src, t = arg

            def poll():
                wd = self.mem['xt'][src][t % 2][0]
                if wd is SENT or wd[0] < t:
                    self.at(0.5, poll)
                    return
                if wd[0] > t:
                    self.violations.append(f'x[slot {src}] of step {t} was overwritten by step {wd[0]} before slot {s} read it')
                elif wd[1] != s:
                    self.violations.append(f'a wave of slot {s} took x_{t} of slot {wd[1]}')
                self.resume(p)
            poll()
        elif kind == 'barrier':
            key, count = arg
            waiting = self.bar.setdefault(key, [])
            waiting.append(p)
            if len(waiting) == count:
                self.bar[key] = []
                for q in waiting:
                    self.at(0.0, (lambda q=q: self.resume(q)))
        elif kind == 'drain':
            def drain():
                if self.pending.get(arg, 0) > 0:
                    self.at(0.2, drain)
                else:
                    self.resume(p)
            drain()
        else:
            raise AssertionError(kind)

    def run(self):
        procs = [self.program(role, j, q) for role in ('A', 'B') for j in range(self.n) for q in (0, 1)]
        for p in procs:
            self.resume(p)
        while self.events and self.now < self.limit:             # (a dead-locked model polls for ever: the clock is the limit)
            self.now, _, fn = heapq.heappop(self.events)
            fn()
        if self.done != len(procs):
            self.violations.append(f'no progress: {self.done} of {len(procs)} half workgroups finished')
        return self.violations

    def program(self, role, j, q):
        who, n, steps = (role, j, q), self.n, self.steps
        a = role == 'A'
        me = 2 * j + q                                        # this half's words of its layer's h / x (and of cI)
        wgi = j if a else n + j                               # the workgroup's words of y1 (q = 0) / y2 (q = 1)
        mine = ('h1', 'x1') if a else ('h2', 'x2')
        fcl, fin = ('y1', 'x2') if q == 0 else ('y2', 'y1')
        slots = [s for s in (0, 1) if self.live[s]]

        def publish(layer, s, t, idx):
            self.store(who, layer, s, t % RING, idx, t)

        def rearm(s, t):
            for layer, idx in ((mine[0], me), (mine[1], me), (fcl, wgi)):
                self.store(who, layer, s, (t + self.ahead) % RING, idx, SENT, rearm_turn=t + self.ahead - RING + 1)

        def form(s, tt):
            if tt < steps:
                self.store(who, 'cI', s, tt % RING, me, tt)

        def x_word(s, t):                                     # which slot's tagged word a wave of slot s looks at (the kernel: its own)
            return ('xtag', (s, s if s == 0 else self.x_from, t))

        sub = lambda layer, s: self.subset(who, layer, s)
        for s in slots:
            if a:
                yield ('gather', ('cI', s, 0, sub('cI', s))); yield ('work', 0.5)
            else:
                for tt in range(1 + self.cond_lead):
                    form(s, tt)
        for t in range(steps):
            if self.drain:
                yield ('drain', who)
            if self.use_barrier:
                yield ('barrier', ((role, j, 'top'), 2))
            if a:
                for s in (slots if not self.wait_empty else (0, 1)):
                    if t > 0:
                        yield x_word(s, t - 1)
                    if s in slots:
                        yield ('work', 0.3)
                        publish('x1', s, t, me); publish('h1', s, t, me)
                for s in slots:
                    yield ('gather', ('h1', s, t, sub('h1', s))); yield ('work', 0.5)
            else:
                for s in slots:
                    if t > 0:
                        yield x_word(s, t - 1)
                    yield ('gather', ('x1', s, t, sub('x1', s))); yield ('work', 0.6)
                    publish('x2', s, t, me); publish('h2', s, t, me)
            for s in slots:                                   # this half's fc tile, then its re-arm (behind its last sentinel poll of the step in this slot)
                yield ('gather', (fin, s, t, sub(fin, s))); yield ('work', 0.3); publish(fcl, s, t, wgi)
                rearm(s, t)
            if a:
                if t + 1 < steps:
                    for s in slots:
                        yield ('gather', ('cI', s, t + 1, sub('cI', s))); yield ('work', 0.5)
            else:
                if j == 0:                                    # the sampling workgroup reads ALL partial tiles of y2[s](t); its waves meet in an LDS barrier
                    for s in slots:
                        yield ('gather', ('y2', s, t, None)); yield ('work', 0.4)
                        yield ('barrier', ((role, j, 'smp', s), 2))
                        if q == 1:
                            yield ('work', 0.4)
                            self.store(who, 'xt', s, t % 2, 0, (t, s))
                for s in slots:
                    yield ('gather', ('h2', s, t, sub('h2', s))); yield ('work', 0.5)
                for s in slots:
                    form(s, t + 1 + self.cond_lead)


def test_two_groups_exchange_is_safe_under_adversarial_timing():
    for seed in range(8):
        for n in (1, 2, 3):
            for density in (0.15, 0.5, 1.0):
                for second in ('full', 'ragged', 'empty'):
                    v = TwoGroupSim(seed, n=n, density=density, second=second).run()
                    assert not v, (seed, n, density, second, v[:3])


def test_two_groups_model_detects_the_shortcuts():
    def broken(seeds=100, n=3, density=0.3, **kw):
        return any(TwoGroupSim(seed, n=n, steps=30, density=density, **kw).run() for seed in range(seeds))
    assert broken(drain=False)                          # a missing drain: a late re-arm (or a late cI) of either slot lands on / hides newer data
    assert broken(ahead=1)                              # re-armed one step ahead: the next step's publication can overtake the re-arm
    assert broken(seeds=3, x_from=0)                    # slot 1 looks at slot 0's x word: the right step of the wrong group
    assert broken(seeds=2, second='empty', wait_empty=True, limit=4000.0)     # a slot without a group is waited for: nobody ever publishes there


def test_other_safe_distances_with_two_groups():
    """Also safe (not what the kernel does): three ahead -- per slot the bound of the one-group protocol."""
    for seed in range(6):
        for second in ('full', 'ragged'):
            v = TwoGroupSim(seed, n=2, ahead=3, second=second).run()
            assert not v, (seed, second, v[:3])
