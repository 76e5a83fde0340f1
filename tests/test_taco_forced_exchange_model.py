"""A discrete-event MODEL of the FORCED step order of wrnn_taco_batch_kernel<SMAX, true> (csrc/wrnn_taco_batch.hip, `wrnn_taco_decode_forced`):
the tagged two-parity exchange of tests/test_taco_batch_exchange_model.py (its `Sim`: memory, adversarial store delays, stalls and poller are
reused) with the teacher-forced program.  The PreNet output of every step is in an immutable table before the loop, so a step has NO 'pre1' /
'pre2' / 'mel' vectors and NO poll at its top: it starts at the attention GRU, which stages the previous step's context and attn_h, and a
sentence is live for exactly its own step count ceil(N_s / r) -- nothing that is exchanged ends it.

What the free-running kernel's mel poll did for WAR safety (no workgroup starts step t + 1 before every mel row of step t is out) is gone; the
two parity buffers must now be safe because every wave publishes an LSTM unit ('h1x2', 'h2x3': producers 'all') of every live sentence in every
step and every workgroup polls them.  Checked under the same adversarial timing:

* a poll that succeeds has read the value of ITS step and ITS sentence in every entry;
* all workgroups finish, with ceil(N_s / r) steps per sentence;
* an entry of a sentence that has ended is never written again.

Negative control: ONE buffer per vector instead of two must fail."""
import pytest

from test_taco_batch_exchange_model import Sim

# layers of a forced step in program order (the mel rows go to the caller's buffer only: written, never exchanged)
LAYERS = [('attn_h', 'some'), ('pq', 'some'), ('s', 'some'), ('ctx', 'some'), ('x', 'all'), ('h1x2', 'all'), ('h2x3', 'all')]
READS = {'attn_h': [('ctx', 1), ('attn_h', 1)], 'pq': [('attn_h', 0)], 's': [('pq', 0)], 'ctx': [('s', 0)], 'x': [('ctx', 0)],
         'h1x2': [('x', 0), ('h1x2', 1)], 'h2x3': [('h1x2', 0), ('h2x3', 1)]}
FINAL_READ = [('h2x3', 0)]                                               # the mel projection stages this step's x3


class ForcedSim(Sim):
    """frames[s] ground-truth frames at `r` frames per step: sentence s runs ceil(frames[s] / r) steps."""

    def __init__(self, seed, frames, r, n_wg=4, buffers=2):
        self.frames, self.r = list(frames), r
        steps = [(n + r - 1) // r for n in frames]
        super().__init__(seed, steps, [None] * len(steps), n_wg=n_wg, buffers=buffers)
        self.rows = {name: list(range(n_wg)) if who == 'all' else list(range(max(1, n_wg // 2))) for name, who in LAYERS}
        self.mem = [{name: [[(0, None)] * len(self.rows[name]) for _ in range(buffers)] for name, _ in LAYERS} for _ in range(self.S)]
        self.mel_rows = {}                                               # (sentence, step, workgroup) -> times written

    def program(self, wg):
        live = [True] * self.S
        done = [0] * self.S
        step = 0
        while True:
            for s in range(self.S):
                if live[s] and step >= self.limits[s]:
                    live[s], done[s] = False, step
            if not any(live):
                break
            for name, _ in LAYERS + [('mel', 'some')]:
                reads = FINAL_READ if name == 'mel' else READS[name]
                want = [(s, vec, step - back) for s in range(self.S) if live[s] for vec, back in reads if step - back >= 0]
                if want:
                    yield ('poll', want, None)
                yield ('work', self.rng.choice([0.2, 0.5, 1.0, 4.0]) if self.rng.random() > 0.004 else 150.0)
                if name == 'mel':
                    for s in range(self.S):
                        if live[s]:
                            if step >= self.ends[s]:
                                self.violations.append(f'sentence {s} ended after {self.ends[s]} steps, mel row written for step {step}')
                            self.mel_rows[s, step, wg] = self.mel_rows.get((s, step, wg), 0) + 1
                elif wg in self.rows[name]:
                    for s in range(self.S):
                        if live[s]:
                            yield ('store', s, name, step % self.nbuf, self.rows[name].index(wg), step, (s, name, step, False, wg))
            step += 1
        self.steps_done[wg] = done
        self.done += 1


FRAMES, R = (27, 33, 23, 9, 1), 2                                        # 14, 17, 12, 5 and 1 steps: odd lengths, a single-step sentence


@pytest.mark.parametrize('seed', range(10))
def test_every_sentence_runs_its_own_step_count_and_every_poll_reads_its_step_and_sentence(seed):
    sim = ForcedSim(seed, FRAMES, R)
    assert sim.ends == [14, 17, 12, 5, 1]
    assert sim.run(), (sim.done, sim.steps_done, sim.violations[:3])
    assert all(d == [14, 17, 12, 5, 1] for d in sim.steps_done.values())
    # every workgroup wrote its mel rows once per live step of every sentence, and none past a sentence's end
    assert sim.mel_rows == {(s, k, wg): 1 for s, e in enumerate(sim.ends) for k in range(e) for wg in range(sim.n_wg)}


def test_one_frame_per_step_and_a_single_sentence():
    sim = ForcedSim(3, (20,), 1)
    assert sim.ends == [20] and sim.run(), (sim.done, sim.violations[:3])


def test_the_forced_program_has_no_prenet_or_mel_vectors():
    sim = ForcedSim(0, FRAMES, R)
    assert not {'pre1', 'pre2', 'mel'} & set(sim.mem[0])
    assert all(step >= 0 for _, back in sum(READS.values(), []) for step in [1 - back])


def test_the_model_sees_a_single_buffer_fail():
    """ONE buffer per vector: without the second buffer the LSTM polls do not keep a fast producer of step t + 1 off the entries a slow
    consumer of step t has not staged yet."""
    bad = 0
    for seed in range(10):
        bad += not ForcedSim(seed, FRAMES, R, buffers=1).run()
    assert bad >= 5, bad
