"""A discrete-event MODEL of the 9-bit RAW mode of wrnn_sparse_kernel (csrc/wrnn_sparse.hip, MODE 0), built on SparseFcSim
(tests/test_sparse_exchange_model.py: half workgroups, gathered fc stages, step barrier, every wave waits for x_{t-1}).  What RAW adds:

    every workgroup:  ... fc2 -> publish y2 | fc3: each half polls ITS half of y2(t) (K split over the waves), LDS barrier, publishes its
                      words of the logits (layer 16), RE-ARMS them in entry t + 2 | rnn1: poll cI(t + 1) ...
    sampler s (4 rnn2 workgroups; here min(n, 4)):  each half polls its half of the logits, LDS barrier, samples its segments and publishes
                      their tagged words x_t -- a sampler with no live segment publishes none | poll h2 -> gh | form cI

    consumers of x_{t-1} wait for the tagged word of EVERY live segment, i.e. of every live sampler.

The skew argument "x_t exists => everyone finished step t - 1" now runs through fc3: a sampler samples step t only behind the logits of
EVERY workgroup (its halves together read all 4 n words), which each publish behind their LDS barrier, i.e. behind both halves' y2(t)
polls ... behind the top of step t.  The checks are SparseFcSim's (whatever a consumer accepts carries its step, no re-arm lands on live
data, everybody finishes), plus: every x word a consumer USES carries the step it waited for.  Broken variants show the model detects
the shortcuts the kernel does not take.  A model of the protocol, not of the HIP code (tests/test_gpu_sparse_raw.py)."""
import heapq

from test_duo_exchange_model import RING, SENT
from test_sparse_exchange_model import SparseFcSim


class SparseRawSim(SparseFcSim):
    def __init__(self, seed, n=2, steps=24, density=0.5, lg_ahead=2, lg_site='fc3', live_samplers=None, x_from_all=True, **kw):
        super().__init__(seed, n=n, steps=steps, density=density, **kw)
        self.ns = min(n, 4)
        self.live = self.ns if live_samplers is None else live_samplers
        self.lg_ahead, self.lg_site, self.x_from_all = lg_ahead, lg_site, x_from_all
        ring = lambda producers, entries: [[[SENT] * producers for _ in range(entries)]]
        self.mem['lg'] = ring(4 * n, RING)                    # layer 16: the two halves of every one of the 2 n workgroups
        self.mem['xt'] = ring(2 * self.ns, 2)                 # x_t: one word per sampler half (its segments), two entries, no re-arm

    def resume(self, p):
        try:
            kind, arg = next(p)
        except StopIteration:
            self.done += 1
            return
        if kind == 'xuse':                                   # the consumer takes x_{t} of every live segment: each word must be step t's
            t, idxs = arg
            words = self.mem['xt'][0][t % 2]
            for k in idxs:
                if words[k] != t:
                    self.violations.append(f'xt[{k}] used as step {t} but holds {words[k]}')
            self.resume(p)
        else:
            def again():
                yield (kind, arg)
                yield from p
            SparseFcSim.resume(self, again())

    def run(self):
        procs = [self.program(role, j, q) for role in ('A', 'B') for j in range(self.n) for q in (0, 1)]
        for p in procs:
            self.resume(p)
        while self.events and self.now < 60000.0:
            self.now, _, fn = heapq.heappop(self.events)
            fn()
        if self.done != len(procs):
            self.violations.append(f'no progress: {self.done} of {len(procs)} half workgroups finished')
        return self.violations

    def program(self, role, j, q):
        who, n, steps = (role, j, q), self.n, self.steps
        a = role == 'A'
        me = 2 * j + q
        wgi = j if a else n + j
        mine = ('h1', 'x1') if a else ('h2', 'x2')
        fcl = 'y1' if q == 0 else 'y2'
        live_words = [2 * s + h for s in range(self.live) for h in (0, 1)]
        waited = live_words if self.x_from_all else [k for k in live_words if k < 2]
        sampler = not a and j < self.ns

        def publish(layer, t, idx):
            self.store(who, layer, 0, t % RING, idx, t)

        def rearm(t):
            for layer, idx in ((mine[0], me), (mine[1], me), (fcl, wgi)):
                self.store(who, layer, 0, (t + self.ahead) % RING, idx, SENT, rearm_turn=t + self.ahead - RING + 1)

        def rearm_lg(t):
            self.store(who, 'lg', 0, (t + self.lg_ahead) % RING, 2 * wgi + q, SENT, rearm_turn=t + self.lg_ahead - RING + 1)

        def form(tt):
            if not a and tt < steps:
                self.store(who, 'cI', 0, tt % RING, me, tt)

        sub = lambda layer, m=2 * n: self.subset((who, layer), m)
        if a:
            yield ('pollsub', ('cI', 0, sub('cI'))); yield ('work', 0.5)
        else:
            for tt in range(1 + self.cond_lead):
                form(tt)
        for t in range(steps):
            if self.drain:
                yield ('drain', who)
            if self.lg_site == 'top':
                rearm_lg(t)
            if self.use_barrier:
                yield ('barrier', ((role, j, 'top'), 2))
            if t > 0 and (a or self.tag_all):
                for k in waited:
                    yield ('tag', ('xt', 0, k, t - 1))
                yield ('xuse', (t - 1, live_words))
            if a:
                yield ('work', 0.3)
                publish('x1', t, me); publish('h1', t, me)
                yield ('pollsub', ('h1', t, sub('h1'))); yield ('work', 0.5)
            else:
                yield ('pollsub', ('x1', t, sub('x1'))); yield ('work', 0.6)
                publish('x2', t, me); publish('h2', t, me)
            if q == 0:
                yield ('pollsub', ('x2', t, sub('x2'))); yield ('work', 0.3); publish('y1', t, wgi)
            else:
                yield ('pollsub', ('y1', t, sub('y1'))); yield ('work', 0.3); publish('y2', t, wgi)
            rearm(t)
            # fc3 (dense, every workgroup): this half's K half of y2(t), the LDS barrier, its logit words, their re-arm
            yield ('pollsub', ('y2', t, [k for k in range(2 * n) if k % 2 == q])); yield ('work', 0.4)
            yield ('barrier', ((role, j, 'f3'), 2))
            publish('lg', t, 2 * wgi + q)
            if self.lg_site == 'fc3':
                rearm_lg(t)
            if a:
                if t + 1 < steps:
                    yield ('pollsub', ('cI', t + 1, sub('cI'))); yield ('work', 0.5)
            else:
                if sampler:                                   # this half gathers the logits of the workgroups of its K half; the halves meet in LDS
                    yield ('pollsub', ('lg', t, [k for k in range(4 * n) if (k // 2) % 2 == q])); yield ('work', 0.3)
                    yield ('barrier', ((role, j, 'smp'), 2))
                    yield ('work', 0.6)
                    if j < self.live:
                        self.store(who, 'xt', 0, t % 2, 2 * j + q, t)
                yield ('pollsub', ('h2', t, sub('h2'))); yield ('work', 0.5)
                form(t + 1 + self.cond_lead)


def test_sparse_raw_exchange_is_safe_under_adversarial_timing():
    for seed in range(40):
        for n in (1, 2, 3):
            for density in (0.15, 0.5, 1.0):
                v = SparseRawSim(seed, n=n, steps=24, density=density).run()
                assert not v, (seed, n, density, v[:3])


def test_sparse_raw_exchange_ragged_groups():
    """A group of fewer segments than 4 samplers x 4 waves: samplers without a live segment publish nothing and nobody waits for them."""
    for seed in range(40):
        for n, live in ((2, 1), (3, 1), (3, 2)):
            v = SparseRawSim(seed, n=n, steps=24, density=0.3, live_samplers=live).run()
            assert not v, (seed, n, live, v[:3])


def test_sparse_raw_other_safe_distances():
    """Also safe (not what the kernel does): the logits re-armed three ahead behind the fc3 barrier -- that barrier has seen y2(t) of every
    workgroup, the samplers' included, and a sampler publishes y2(t) only after its sampling of step t - 1."""
    for seed in range(30):
        v = SparseRawSim(seed, n=3, steps=24, density=0.3, lg_ahead=3).run()
        assert not v, (seed, v[:3])


def test_sparse_raw_model_detects_the_shortcuts():
    def broken(n=3, density=0.3, **kw):
        return any(SparseRawSim(seed, n=n, steps=30, density=density, **kw).run() for seed in range(150))
    assert broken(lg_site='top', lg_ahead=3)         # layer 16 re-armed too early: at the top of step t, before anything of step t was seen
    assert broken(drain=False)                       # no drain: a late re-arm lands on the next publication
    assert broken(x_from_all=False)                  # x_t taken from one sampler only: the other samplers' words can still hold step t - 2
