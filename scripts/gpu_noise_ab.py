#!/usr/bin/env python
"""What drawing the sampling noise inside the library is worth on the benchmarked batch: `generate_corpus` on 16 x 641-frame utterances (256 segments x
12,100 steps), 9-bit RAW and MoL, wall time per pass (host clock around the call and a device synchronise) and loop-kernel launches per pass, for
noise_source='device' on one tree and 'library' on another -- each measurement in a fresh process, the two alternating, several rounds, so that the
run-to-run spread of the baseline is reported beside the difference.

    python scripts/gpu_noise_ab.py --baseline-root <checkout of the parent commit, built> [--rounds 3] [--passes 5] [--out profiles/noise_ab.json]
    python scripts/gpu_noise_ab.py --one --root <tree> --mode RAW --noise library     # one measurement: a JSON line (what the driver starts)
"""
import argparse, json, os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--one', action='store_true'); ap.add_argument('--root', default=HERE); ap.add_argument('--baseline-root', default=None)
ap.add_argument('--mode', default='RAW'); ap.add_argument('--noise', default='library'); ap.add_argument('--modes', default='RAW,MOL')
ap.add_argument('--utterances', type=int, default=16); ap.add_argument('--passes', type=int, default=5); ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--out', default=None)
a = ap.parse_args()


def one():
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np, torch
    from wavernn_amd.batch import generate_corpus
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED
    dev = torch.device('cuda', 0)
    m = WaveRNN(**SHIPPED, mode=a.mode)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(0, mode=a.mode).items()}, strict=True)
    m = m.to(dev).eval()
    mels = [torch.from_numpy(random_mel(1234 + u, 641)).unsqueeze(0).to(dev) for u in range(a.utterances)]
    seeds = [77 + u for u in range(a.utterances)]
    ms, launches, loop_ms = [], None, []
    for i in range(a.passes + 1):                      # (the first pass warms up: code objects, the workspace, torch's allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = generate_corpus(m, mels, 11000, 550, True, seeds, noise_source=a.noise, finish='own', check=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        e = m._loop_engine()
        e.status()
        if i:
            ms.append(dt); loop_ms.append(e.last_loop_ms())
        launches = e.last_run_info()
    print(json.dumps(dict(root=os.path.relpath(os.path.abspath(a.root), HERE), mode=a.mode, noise=a.noise, ms_per_pass=[round(x, 2) for x in ms],
                          loop_kernel_ms=[round(x, 2) for x in loop_ms], kernel=launches['kernel'], launches_per_pass=launches['launches'],
                          slab_steps=launches['slab_steps'], samples=int(sum(len(o) for o in outs if o is not None)))), flush=True)


def driver():
    import statistics
    base = a.baseline_root or HERE
    rows = []
    for mode in a.modes.split(','):
        for r in range(a.rounds):
            for root, noise in ((base, 'device'), (HERE, 'library')):          # alternating, every measurement in a process of its own
                res = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', '--root', root, '--mode', mode, '--noise', noise,
                                      '--utterances', str(a.utterances), '--passes', str(a.passes)], stdout=subprocess.PIPE, text=True, timeout=600)
                if res.returncode != 0:
                    raise SystemExit(f'{root} {mode} {noise}: exit status {res.returncode}')
                row = json.loads(res.stdout.strip().splitlines()[-1]); row['round'] = r
                rows.append(row); print(json.dumps(row), flush=True)
    summary = []
    for mode in a.modes.split(','):
        s = dict(mode=mode)
        for noise in ('device', 'library'):
            per_round = [statistics.median(x['ms_per_pass']) for x in rows if x['mode'] == mode and x['noise'] == noise]
            every = [v for x in rows if x['mode'] == mode and x['noise'] == noise for v in x['ms_per_pass']]
            loop = [v for x in rows if x['mode'] == mode and x['noise'] == noise for v in x['loop_kernel_ms']]
            s[noise] = dict(median_ms=round(statistics.median(every), 2), min_ms=round(min(every), 2), max_ms=round(max(every), 2),
                            round_medians_ms=[round(v, 2) for v in per_round], loop_kernel_median_ms=round(statistics.median(loop), 2),
                            launches_per_pass=[x['launches_per_pass'] for x in rows if x['mode'] == mode and x['noise'] == noise][0])
        s['baseline_spread_ms'] = round(max(s['device']['round_medians_ms']) - min(s['device']['round_medians_ms']), 2)
        s['library_minus_device_ms'] = round(s['library']['median_ms'] - s['device']['median_ms'], 2)
        summary.append(s); print(json.dumps(s), flush=True)
    if a.out:
        json.dump(dict(what='generate_corpus, 16 x 641 frames = 256 segments x 12,100 steps; wall ms per pass, one warm-up pass per process',
                       baseline_root=os.path.relpath(os.path.abspath(base), HERE), passes=a.passes, rounds=a.rounds, summary=summary, runs=rows),
                  open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    one() if a.one else driver()
