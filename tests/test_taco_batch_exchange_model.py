"""A discrete-event MODEL of wrnn_taco_batch_kernel's exchange (csrc/wrnn_taco_batch.hip): the tagged two-parity exchange of
wrnn_taco_resident_kernel (tests/test_taco_exchange_model.py) with a SENTENCE dimension.  Every sentence has its own entries -- per vector two
buffers by step parity, an entry an 8-byte word {value, tag = step + 1} written by ONE store -- and a step runs layer by layer over all LIVE
sentences: a workgroup polls the inputs of every live sentence together, then publishes its rows of every live sentence.  Sentences END at
different steps, in two ways: at their own step limit, or because the mel block polled at the top of a step says "stop".  No workgroup is
told that a sentence has ended: each derives the live mask from the limits and from the mel words it polled itself.

Checked under adversarial timing (a store lands after a random delay, out of program order; every layer of every workgroup takes a random
time, now and then a stall longer than two whole steps):

* a poll that succeeds has read the value of ITS step and ITS sentence in every entry;
* all workgroups finish, with the same step count per sentence;
* an entry of a sentence that has ended is never written again.

Negative controls, each of which must fail: ONE buffer per vector instead of two, and a workgroup that derives its live mask one step late
(it polls for a sentence whose producers consider it ended: the dead-lock the kernel rules out by deriving the mask everywhere from the same
words with the same code).  A model of the protocol, not of the HIP code -- tests/test_gpu_taco_batch.py covers that."""
import heapq
import random

import pytest

# layers of a decoder step in program order: (name, producers) -- 'all' = every workgroup owns rows, 'some' = only the first workgroups do
LAYERS = [('pre1', 'some'), ('pre2', 'some'), ('attn_h', 'some'), ('pq', 'some'), ('s', 'some'), ('ctx', 'some'), ('x', 'all'),
          ('h1x2', 'all'), ('h2x3', 'all'), ('mel', 'some')]
# what a layer stages: (vector, 0 = this step / 1 = the previous step's).  The mel block of the previous step is polled at the TOP of a step
# (stop test, then the first prenet layer's input), so 'pre1' stages nothing more.
READS = {'pre1': [], 'pre2': [('pre1', 0)], 'attn_h': [('ctx', 1), ('attn_h', 1), ('pre2', 0)], 'pq': [('attn_h', 0)],
         's': [('pq', 0)], 'ctx': [('s', 0)], 'x': [('ctx', 0)], 'h1x2': [('x', 0), ('h1x2', 1)], 'h2x3': [('h1x2', 0), ('h2x3', 1)],
         'mel': [('h2x3', 0)]}


class Sim:
    """limits[s]: step limit of sentence s; stops[s]: the mel block of step stops[s] - 1 says "stop" (None: never), so the sentence ends
    after stops[s] steps if its limit does not end it first.  late_wg: that workgroup applies every stop one step late."""

    def __init__(self, seed, limits, stops, n_wg=4, buffers=2, late_wg=None):
        self.rng = random.Random(seed)
        self.n_wg, self.nbuf, self.late_wg = n_wg, buffers, late_wg
        self.limits, self.stops, self.S = list(limits), list(stops), len(limits)
        self.ends = [min(l, st) if st is not None else l for l, st in zip(self.limits, self.stops)]
        self.rows = {name: list(range(n_wg)) if who == 'all' else list(range(max(1, n_wg // 2))) for name, who in LAYERS}
        # mem[sentence][vector][buffer][row] = (tag, value)
        self.mem = [{name: [[(0, None)] * len(self.rows[name]) for _ in range(buffers)] for name, _ in LAYERS} for _ in range(self.S)]
        self.now, self.events, self.seq, self.pending = 0.0, [], 0, 0
        self.violations, self.done, self.steps_done, self.idle_polls = [], 0, {}, 0

    def at(self, dt, fn, poll=False):
        self.seq += 1
        self.pending += not poll                                          # stores in flight and work: what can still change the memory
        heapq.heappush(self.events, (self.now + dt, self.seq, poll, fn))

    def store(self, s, vec, buf, row, step, value):
        if step >= self.ends[s]:
            self.violations.append(f'sentence {s} ended after {self.ends[s]} steps, {vec} written for step {step}')

        def land():
            self.mem[s][vec][buf][row] = (step + 1, value)
        self.at(self.rng.choice([0.1, 0.3, 1.0, 2.0, 6.0]), land)

    def program(self, wg):
        live = [True] * self.S
        done = [0] * self.S
        pending_stop = [False] * self.S                                  # (late_wg: a stop seen, applied one step later)
        got = {}
        step = 0
        while True:
            for s in range(self.S):
                if live[s] and (step >= self.limits[s] or pending_stop[s]):
                    live[s], done[s] = False, step
            if not any(live):
                break
            if step > 0:
                got.clear()
                yield ('poll', [(s, 'mel', step - 1) for s in range(self.S) if live[s]], got)
                for s in range(self.S):
                    if live[s] and all(v[3] for v in got[s, 'mel']):       # every polled word of the block says "stop"
                        if wg == self.late_wg:
                            pending_stop[s] = True
                        else:
                            live[s], done[s] = False, step
                if not any(live):
                    break
            for name, _ in LAYERS:
                want = [(s, vec, step - back) for s in range(self.S) if live[s] for vec, back in READS[name] if step - back >= 0]
                if want:
                    yield ('poll', want, None)
                # (a rare long stall -- a pre-empted or throttled CU: longer than two whole steps of the others)
                yield ('work', self.rng.choice([0.2, 0.5, 1.0, 4.0]) if self.rng.random() > 0.004 else 150.0)
                if wg in self.rows[name]:
                    for s in range(self.S):
                        if live[s]:
                            stop = name == 'mel' and self.stops[s] is not None and step == self.stops[s] - 1
                            yield ('store', s, name, step % self.nbuf, self.rows[name].index(wg), step, (s, name, step, stop, wg))
            step += 1
        self.steps_done[wg] = done
        self.done += 1

    def run(self):
        procs = [self.program(wg) for wg in range(self.n_wg)]
        blocked = {}

        def advance(i):
            for act in procs[i]:
                if act[0] == 'work':
                    self.at(act[1], lambda i=i: advance(i))
                    return
                if act[0] == 'store':
                    self.store(*act[1:])
                    continue
                blocked[i] = act
                self.at(0.0, lambda i=i: poll(i), poll=True)
                return

        def poll(i):
            _, want, got = blocked[i]
            if all(t == src + 1 for s, vec, src in want for t, _ in self.mem[s][vec][src % self.nbuf]):
                for s, vec, src in want:
                    entries = self.mem[s][vec][src % self.nbuf]
                    for row, (_, val) in enumerate(entries):
                        if val[:3] != (s, vec, src) or val[4] != self.rows[vec][row]:
                            self.violations.append(f'workgroup {i} staged {val} for {vec} of sentence {s}, step {src}')
                    if got is not None:
                        got[s, vec] = [val for _, val in entries]
                del blocked[i]
                self.idle_polls = 0
                advance(i)
            else:
                self.idle_polls = self.idle_polls + 1 if self.pending == 0 else 0      # nothing in flight can still change the memory
                self.at(0.4, lambda i=i: poll(i), poll=True)

        for i in range(self.n_wg):
            self.at(self.rng.random(), lambda i=i: advance(i))
        guard = 0
        while self.events and guard < 2_000_000:
            guard += 1
            self.now, _, is_poll, fn = heapq.heappop(self.events)
            self.pending -= not is_poll
            fn()
            if self.idle_polls > 2 * self.n_wg:
                break                                                     # no progress: only pollers left, spinning for a tag that never comes
        same = all(d == self.ends for d in self.steps_done.values())
        return self.done == self.n_wg and not self.violations and same


# three sentences: one ends by its limit, one by a "stop" in the polled mel, one has both and the stop comes first; a fourth outlives them
LIMITS, STOPS = (14, 30, 22, 9), (None, 17, 12, None)


@pytest.mark.parametrize('seed', range(10))
def test_sentences_end_on_their_own_and_every_poll_reads_its_step_and_sentence(seed):
    sim = Sim(seed, LIMITS, STOPS)
    assert sim.ends == [14, 17, 12, 9]
    assert sim.run(), (sim.done, sim.steps_done, sim.violations[:3])
    assert all(d == [14, 17, 12, 9] for d in sim.steps_done.values())


def test_a_single_sentence_is_the_single_kernel_protocol():
    sim = Sim(1, (20,), (None,))
    assert sim.run(), (sim.done, sim.violations[:3])


def test_the_model_sees_a_single_buffer_fail():
    """ONE buffer per vector: a fast producer of step t + 1 overwrites entries a slow consumer of step t has not staged yet."""
    bad = 0
    for seed in range(10):
        bad += not Sim(seed, LIMITS, STOPS, buffers=1).run()
    assert bad >= 5, bad


def test_the_model_sees_a_late_live_mask_fail():
    """One workgroup applies a sentence's stop one step late: it polls (and publishes) for a sentence that every other workgroup has ended --
    entries written past the end, and a poll for words that never come."""
    bad = 0
    for seed in range(10):
        bad += not Sim(seed, LIMITS, STOPS, late_wg=1).run()
    assert bad == 10, bad
