#!/usr/bin/env python
"""A/B of the two loop kernels that run a generic pack, on one MI355X and one build: `wrnn_tile_kernel` (algo 'tile': one workgroup per 16 segments, MFMA,
csrc/wrnn_tile.hip) against `wrnn_generic_kernel` (algo 'auto': one workgroup per segment, fmaf chains, csrc/wrnn_generic.hip: the yardstick).

    geometries   mol256: MoL, rnn = fc = 256, feat 80, aux 32        raw10: RAW 10 bits (1024 classes), rnn = fc = 512, feat 80, aux 32
    segments     B = 1, 16, 64, 256, 1024;  T = 2000 steps, every step live (stride 21, hop 8)

The timer is `wrnn_timer` around the loop launch (`LoopEngine.last_loop_ms`); the noise is the library's (wrnn_options.noise_lib: drawn into the workspace
before the timed launch, the same stream for both kernels), weights are random-init.  Per (geometry, B): one warm-up of each kernel, then `--reps` timed
runs of each, alternating; minimum and median, us per step, and tile's throughput ratio = generic / tile.  The samples of the two kernels are compared
(RAW: how many differ; MoL: max abs difference) and reported, not asserted: this is a measurement.

Every (geometry, B) runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python scripts/gpu_tile_ab.py --out profiles/tile_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEOMETRIES = dict(mol256=dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128),
                  raw10=dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=10, feat_dims=80, res_out_dims=128))
SEGMENTS = (1, 16, 64, 256, 1024)
T, HOP, STRIDE = 2000, 8, 21
SEED = 0x5EED0123456789AB


def one(geometry, B, reps):
    """One (geometry, B) on the device of this process -> a dict."""
    import numpy as np
    import torch
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.synthetic import random_state_dict
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda', 0)
    g = GEOMETRIES[geometry]
    sd = random_state_dict(5, compute_dims=8, res_blocks=1, **g)
    eng = LoopEngine(sd, g['mode'], device=dev)
    M, A = g['feat_dims'], g['res_out_dims'] // 4
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    rs = np.random.RandomState(1)
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, M)).astype(np.float32)).to(dev)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 4 * A)).astype(np.float32)).to(dev)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32)
    kernels = dict(tile='wrnn_tile_kernel', auto='wrnn_generic_kernel')

    def run(algo):
        out = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, algo=algo, noise_seed=SEED)
        assert eng.last_loop_kernel() == kernels[algo], (algo, eng.last_loop_kernel())
        return out, eng.last_loop_ms()

    outs = {algo: run(algo)[0].cpu().numpy() for algo in ('auto', 'tile')}          # warm-up, and the samples
    ms = dict(auto=[], tile=[])
    for _ in range(reps):
        for algo in ('auto', 'tile'):
            ms[algo].append(run(algo)[1])
    us = lambda v: round(1000.0 * v / T, 3)
    res = dict(geometry=geometry, B=B, T=T, reps=reps, workgroups=dict(generic=B, tile=-(-B // 16)),
               generic_us_per_step=dict(min=us(min(ms['auto'])), median=us(statistics.median(ms['auto']))),
               tile_us_per_step=dict(min=us(min(ms['tile'])), median=us(statistics.median(ms['tile']))),
               tile_speedup_min=round(min(ms['auto']) / min(ms['tile']), 3),
               tile_speedup_median=round(statistics.median(ms['auto']) / statistics.median(ms['tile']), 3))
    if g['mode'] == 'MOL':
        res['samples_max_abs_diff'] = float(np.abs(outs['tile'] - outs['auto']).max())
    else:
        res['samples_differing'] = int(np.count_nonzero(outs['tile'] != outs['auto']))
        res['samples'] = int(outs['tile'].size)
    res['device'] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per (geometry, B) child process')
    ap.add_argument('--one', nargs=2, metavar=('GEOMETRY', 'B'), help='(a child) run one case and print its JSON line')
    a = ap.parse_args()
    if a.one:
        print('TILE_AB ' + json.dumps(one(a.one[0], int(a.one[1]), a.reps)), flush=True)
        return
    rows = []
    for geometry in GEOMETRIES:
        for B in SEGMENTS:
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--one', geometry, str(B), '--reps', str(a.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('TILE_AB ')]
            if p.returncode != 0 or not line:
                print(p.stdout[-4000:])
                raise SystemExit(f'{geometry} B={B}: the child ended with status {p.returncode}; nothing more is started')
            rows.append(json.loads(line[-1][len('TILE_AB '):]))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=rows[0]['device'], T=T, hop=HOP, stride=STRIDE, reps=a.reps, geometries=GEOMETRIES,
               timing='wrnn_timer around the loop launch (LoopEngine.last_loop_ms), the two kernels alternating, warm, library noise; us per step = ms / T',
               yardstick='wrnn_generic_kernel (algo auto); tile_speedup = generic / tile', rows=[{k: v for k, v in r.items() if k != 'device'} for r in rows])
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
