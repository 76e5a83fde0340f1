#!/usr/bin/env python
"""Where one pass of the benchmarked workload spends its time outside the loop kernel (16 x 641-frame utterances through generate_corpus, MoL,
device noise, finish='own': what `bench.py --gpus 1` times):
    python scripts/gpu_pass_breakdown.py --label parent --out profiles/pass_breakdown_parent.json [--prune 0.95 --prune-linear] [--set pre_batched=0 ...]
The phases of a pass are timed from OUTSIDE (wrappers around PreEngine.upsample_many, rng.draw_steps, LoopEngine.run_segments, post.unfold_on_device and
the copy into the pinned buffer), so the same script measures a checkout that knows nothing of it.  Per phase: `host_ms` = until the call returns (the
work is only queued), `done_ms` = until the device has finished it.  The device is synchronised around every phase ONLY here, in this diagnostic mode;
`free_pass_ms` is the pass as the benchmark runs it (no wrapper, one synchronisation at the end), `outside_loop_ms` = that minus the loop kernels' own time.
The kernel time line (gaps between the loop launches included) comes from a separate run:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gpu_pass_breakdown.py --trace-only"""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument('--label', default='parent'); ap.add_argument('--out', default=None)
ap.add_argument('--utterances', type=int, default=16); ap.add_argument('--frames', type=int, default=641); ap.add_argument('--passes', type=int, default=5)
ap.add_argument('--prune', type=float, default=0.0); ap.add_argument('--prune-linear', action='store_true')
ap.add_argument('--set', nargs='*', default=[], metavar='ATTR=INT', help='model attributes (pre_batched, pre_streams, slab_prep_split, post_tables_early, ...)')
ap.add_argument('--trace-only', action='store_true', help='one warm-up pass and one plain pass, nothing else (for a kernel trace)')
ap.add_argument('--trace-csv', default=None, help='summarise the kernel trace of a --trace-only run (its last pass) and leave: needs no device')
a = ap.parse_args()
if a.trace_csv:
    import csv
    rows = sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(open(a.trace_csv))), key=lambda r: r[1])
    ends = [i for i, r in enumerate(rows) if 'wrnn_post_kernel' in r[0]]
    last = rows[ends[-2] + 1:ends[-1] + 1] if len(ends) >= 2 else rows         # the last pass: behind the unfold of the pass before, up to its own
    is_loop = lambda n: any(k in n for k in ('wrnn_duo_kernel', 'wrnn_chain_kernel', 'wrnn_sparse_kernel', 'wrnn_loop_kernel'))
    t0, busy_to, line, loop_us, other_us, idle_us, gaps = last[0][1], last[0][1], [], 0.0, 0.0, 0.0, []
    prev_loop_end = None
    for n, s, e in last:
        short = n.split('(')[0].split('<')[0].split('::')[-1][:48]
        gap = max(0, s - busy_to) / 1e3
        idle_us += gap
        line.append(dict(kernel=short, start_us=round((s - t0) / 1e3, 1), dur_us=round((e - s) / 1e3, 1), idle_before_us=round(gap, 1)))
        if is_loop(n):
            loop_us += (e - s) / 1e3
            if prev_loop_end is not None:
                gaps.append(round((s - prev_loop_end) / 1e3, 1))
            prev_loop_end = e
        else:
            other_us += (e - s) / 1e3
        busy_to = max(busy_to, e)
    first_loop = next(r for r in last if is_loop(r[0]))
    last_loop = [r for r in last if is_loop(r[0])][-1]
    res = dict(label=a.label, dispatches=len(last), span_us=round((last[-1][2] - t0) / 1e3, 1), loop_kernels_us=round(loop_us, 1), other_kernels_us=round(other_us, 1),
               device_idle_us=round(idle_us, 1), before_first_loop_us=round((first_loop[1] - t0) / 1e3, 1), gaps_between_loop_launches_us=gaps,
               after_last_loop_us=round((last[-1][2] - last_loop[2]) / 1e3, 1),
               time_line=line[:400])
    print(json.dumps({k: v for k, v in res.items() if k != 'time_line'}))
    if a.out:
        json.dump(res, open(a.out, 'w'), indent=1)
    sys.exit(0)
from wavernn_amd import pre as _pre, post as _post, rng as _rng, engine as _engine, batch as _batch
from wavernn_amd.model import WaveRNN
from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED
dev = torch.device('cuda', 0)
sd = random_state_dict(0, mode='MOL')
if a.prune > 0:
    from wavernn_amd.prune import block_prune_state_dict
    sd, _ = block_prune_state_dict(sd, a.prune, (16, 1), linear=a.prune_linear)
m = WaveRNN(**SHIPPED, mode='MOL'); m.num_params = lambda *x, **k: 0
m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True); m = m.to(dev).eval()
for kv in a.set:
    k, v = kv.split('='); setattr(m, k, int(v))
mels = [torch.from_numpy(random_mel(1234 + u, a.frames)).unsqueeze(0).to(dev) for u in range(a.utterances)]
eng = m._loop_engine()


def one_pass():
    torch.manual_seed(12345)
    outs = _batch.generate_corpus(m, mels, 11000, 550, True, None, noise_source='device', finish='own', check=False)
    eng.status()
    return outs


def timed_pass():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    outs = one_pass()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, outs


one_pass(); one_pass()
if a.trace_only:
    one_pass(); torch.cuda.synchronize(); sys.exit(0)
free, loop = [], []
for _ in range(a.passes):
    dt, outs = timed_pass()
    free.append(dt); loop.append(eng.last_loop_ms())
n_samples = sum(len(o) for o in outs)

# ---- the diagnostic mode: every phase between two synchronisations
phases = {}


def wrap(owner, name, phase):
    fn = getattr(owner, name)

    def inner(*args, **kw):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn(*args, **kw)
        t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
        p = phases.setdefault(phase, dict(host_ms=0.0, done_ms=0.0, calls=0))
        p['host_ms'] += (t1 - t0) * 1e3; p['done_ms'] += (t2 - t0) * 1e3; p['calls'] += 1
        return r
    setattr(owner, name, inner)
    return fn


orig_copy = torch.Tensor.copy_


def copy_(self, src, non_blocking=False):
    if not (self.is_pinned() and src.is_cuda):
        return orig_copy(self, src, non_blocking)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = orig_copy(self, src, non_blocking)
    t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
    p = phases.setdefault('d2h', dict(host_ms=0.0, done_ms=0.0, calls=0, bytes=0))
    p['host_ms'] += (t1 - t0) * 1e3; p['done_ms'] += (t2 - t0) * 1e3; p['calls'] += 1; p['bytes'] += src.numel() * src.element_size()
    return r


wrap(_pre.PreEngine, 'upsample_many', 'pre_loop')
wrap(_rng, 'draw_steps', 'noise_draw')
wrap(_engine.LoopEngine, 'run_segments', 'loop_call')
wrap(_post, 'unfold_on_device', 'post_unfold')
torch.Tensor.copy_ = copy_
diag = []
for _ in range(a.passes):
    dt, _o = timed_pass()
    diag.append(dt)
torch.Tensor.copy_ = orig_copy
for p in phases.values():
    for k in ('host_ms', 'done_ms'):
        p[k] = round(p[k] / a.passes, 4)
    p['calls'] //= a.passes
    if 'bytes' in p:
        p['bytes'] //= a.passes
med = lambda v: float(np.median(v))
known = sum(p['done_ms'] for p in phases.values())
info = eng.last_run_info()
res = dict(label=a.label, workload=dict(utterances=a.utterances, frames=a.frames, mode='MOL', prune=a.prune, prune_linear=a.prune_linear, settings=a.set),
           kernel=info['kernel'], launches=info['launches'], slab_steps=info['slab_steps'], samples=n_samples,
           free_pass_ms=[round(x, 3) for x in free], free_pass_ms_median=round(med(free), 3), loop_kernel_ms_median=round(med(loop), 3),
           outside_loop_ms=round(med(free) - med(loop), 3), diagnostic_pass_ms_median=round(med(diag), 3), phases=phases,
           plan_tables_and_rest_ms=round(med(diag) - known, 3),
           note='phases: synchronised around each call (diagnostic mode only); loop_call.done_ms holds the loop kernels AND what the library queues between them; '
                'plan_tables_and_rest_ms = the diagnostic pass minus the wrapped phases (plan, tables, allocations, eng.status)')
print(json.dumps(res), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, 'w'), indent=1)
