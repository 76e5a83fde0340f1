"""A discrete-event MODEL of wrnn_tile_wide_kernel's hand-off (csrc/wrnn_tile_wide.hip): the W workgroups of one tile, S matrix stages per step, after every
stage an all-gather of the stage's output vector through ONE buffer per (tile, stage) and W flag words per stage.  Per member, step t, stage s:

    compute its rows | store its slice (write-through) | DRAIN its stores | flag[s][me] = epoch(t, s) = t S + s + 1 |
    wait until flag[s][*] == epoch | read every member's slice of buffer s | the reads have LANDED (they feed LDS in front of a barrier) | next stage

The flag words are zeroed in front of every launch and the epochs count within the launch.  Checked under adversarial timing -- every store, flag and read
lands after a random delay, out of order, now and then later than ten whole steps; only a drain waits for them; members run at very different speeds --:
no member ever reads a slice that is not of its (launch, step, stage), and every member finishes.  The shortcuts the kernel must not take are shown to
break exactly that, so the model is not vacuous.  A model of the protocol, not of the HIP code (tests/test_gpu_tile_wide.py runs that)."""
import heapq
import random

import pytest


class WideSim:
    """One tile's cluster.  Memory: buf[b][member] = the tag (launch, step, stage) of the slice that member last landed in buffer b; flag[s][member]."""

    def __init__(self, seed, W, S, steps=12, launches=1, empty=(), drain_stores=True, finish_reads=True, shared_buffers=False, zero_flags=True):
        self.rng = random.Random(seed)
        self.W, self.S, self.steps, self.launches, self.empty = W, S, steps, launches, set(empty)
        self.drain_stores, self.finish_reads, self.shared, self.zero_flags = drain_stores, finish_reads, shared_buffers, zero_flags
        self.buf = [[None] * W for _ in range(S)]
        self.flag = [[0] * W for _ in range(S)]
        self.violations = []

    def bufidx(self, s):
        return s // 2 * 2 if self.shared else s         # the shortcut: stages 2 i and 2 i + 1 in one buffer

    def delay(self, scale=1.0):
        d = self.rng.expovariate(1.0 / scale)
        if self.rng.random() < 0.03:
            d += 10.0 * self.S * self.rng.random()       # now and then: later than ten whole steps (a stage's work is ~1)
        return d

    def at(self, when, fn):
        self.seq += 1
        heapq.heappush(self.events, (when, self.seq, fn))

    def program(self, launch, m):
        speed = self.rng.choice((0.2, 1.0, 5.0))         # uneven members
        for t in range(self.steps):
            for s in range(self.S):
                tag, epoch, b = (launch, t, s), t * self.S + s + 1, self.bufidx(s)
                yield ('work', speed * self.rng.random())
                if m not in self.empty:
                    yield ('store', b, m, tag)
                if self.drain_stores:
                    yield ('drain', 'stores')
                yield ('flag', s, m, epoch)              # a member with an empty share still signals
                yield ('wait', s, epoch)
                for j in range(self.W):
                    if j not in self.empty:
                        yield ('read', b, j, tag)
                if self.finish_reads:
                    yield ('drain', 'reads')

    def run_launch(self, launch):
        self.events, self.seq, self.now, self.done = [], 0, 0.0, 0
        pending = [dict(stores=0, reads=0) for _ in range(self.W)]
        waiting = {}                                      # member -> what it waits for
        last_flag = {}                                    # (stage, member) -> landing time of its last flag store: one address, stores land in order
        procs = [self.program(launch, m) for m in range(self.W)]

        def wake():
            for m, cond in list(waiting.items()):
                if cond():
                    del waiting[m]
                    resume(m)

        def resume(m):
            while True:
                try:
                    cmd = next(procs[m])
                except StopIteration:
                    self.done += 1
                    return
                if cmd[0] == 'work':
                    self.at(self.now + cmd[1], lambda m=m: resume(m))
                    return
                if cmd[0] == 'store':
                    _, b, j, tag = cmd
                    pending[m]['stores'] += 1

                    def land(b=b, j=j, tag=tag, m=m):
                        self.buf[b][j] = tag
                        pending[m]['stores'] -= 1
                        wake()
                    self.at(self.now + self.delay(), land)
                elif cmd[0] == 'flag':
                    _, s, j, epoch = cmd
                    when = max(self.now + self.delay(0.3), last_flag.get((s, j), 0.0) + 1e-6)
                    last_flag[(s, j)] = when

                    def land(s=s, j=j, epoch=epoch):
                        self.flag[s][j] = epoch
                        wake()
                    self.at(when, land)
                elif cmd[0] == 'read':
                    _, b, j, want = cmd
                    pending[m]['reads'] += 1

                    def land(b=b, j=j, want=want, m=m):
                        if self.buf[b][j] != want:
                            self.violations.append(f'member {m} read {self.buf[b][j]} of member {j} in buffer {b}, wanted {want}')
                        pending[m]['reads'] -= 1
                        wake()
                    self.at(self.now + self.delay(), land)
                elif cmd[0] == 'drain':
                    key = cmd[1]
                    if pending[m][key]:
                        waiting[m] = lambda m=m, key=key: pending[m][key] == 0
                        return
                elif cmd[0] == 'wait':
                    _, s, epoch = cmd
                    cond = lambda s=s, epoch=epoch: all(f == epoch for f in self.flag[s])
                    if not cond():
                        waiting[m] = cond
                        return

        for m in range(self.W):
            resume(m)
        while self.events:
            self.now, _, fn = heapq.heappop(self.events)
            fn()
        if self.done != self.W:
            self.violations.append(f'launch {launch}: {self.W - self.done} of {self.W} members wait forever')

    def run(self):
        for launch in range(self.launches):
            if self.zero_flags:                          # the memset in front of every launch (everything of the launch before has landed: a kernel boundary)
                self.flag = [[0] * self.W for _ in range(self.S)]
            self.run_launch(launch)
            if self.violations:
                break
        return self.violations


SEEDS = range(40)
SHAPES = [(W, S) for W in (2, 4, 8) for S in (5, 6)]


@pytest.mark.parametrize('W, S', SHAPES)
def test_the_kernels_rules_are_safe(W, S):
    for seed in SEEDS:
        assert WideSim(seed, W, S).run() == [], (W, S, seed)


@pytest.mark.parametrize('W, S', SHAPES)
def test_members_with_an_empty_share_still_signal_and_nothing_waits_forever(W, S):
    for seed in SEEDS:
        for empty in ((W - 1,), tuple(range(1, W))):    # the last member idle; everyone but member 0 idle (fc = 33 at W = 8, 2-class RAW)
            assert WideSim(seed, W, S, empty=empty).run() == [], (W, S, seed, empty)


@pytest.mark.parametrize('W, S', SHAPES)
def test_two_launches_on_one_workspace_are_safe_when_the_flags_are_zeroed(W, S):
    for seed in SEEDS:
        assert WideSim(seed, W, S, steps=6, launches=3).run() == [], (W, S, seed)


def broken(**kw):
    return sum(bool(WideSim(seed, W, S, **kw).run()) for seed in SEEDS for W, S in SHAPES)


def test_publishing_before_the_previous_copy_out_has_finished_is_detected():
    """The reads of stage s - 1 still in flight when the member goes on to publish and signal stage s: nothing holds the others back from coming round to
    that buffer again."""
    assert broken(finish_reads=False) > 0


def test_signalling_before_the_payload_is_drained_is_detected():
    assert broken(drain_stores=False) > 0


def test_one_buffer_for_two_consecutive_stages_is_detected():
    assert broken(shared_buffers=True) > 0


def test_epochs_that_are_not_reset_between_launches_are_detected():
    """The flags of the launch before hold the epochs of its LAST step.  Under the kernel's equality match a later launch's member takes them for its own
    where that is the step it is in and the word's owner has not stored yet: launches of one step, whose epochs are the same every time (a longer launch
    overwrites every word with smaller epochs on its way there; a workspace never zeroed at all holds anything).  Zeroing in front of every launch is what
    makes the first wait of every stage a wait for THIS launch's store."""
    assert broken(steps=1, launches=4, zero_flags=False) > 0
    assert broken(steps=1, launches=4) == 0


def test_the_epoch_is_never_zero_and_strictly_increases():
    for S in (5, 6):
        epochs = [t * S + s + 1 for t in range(50) for s in range(S)]
        assert epochs[0] == 1 and all(b == a + 1 for a, b in zip(epochs, epochs[1:]))
