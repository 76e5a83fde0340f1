#!/usr/bin/env python
"""A/B of `wrnn_tile_wide_kernel` (algo 'tile' with clusters = W: the rows of every matrix stage of a tile of 16 segments on W = 2, 4, 8 workgroups that hand the
stage's output to one another, csrc/wrnn_tile_wide.hip) against `wrnn_tile_kernel` (algo 'tile', one workgroup per tile, csrc/wrnn_tile.hip -- the yardstick,
"width 1"), on one MI355X, one build and one pack per leg.  The method of scripts/gpu_tile_bf16_ab.py.

    legs       mol256   MoL, rnn = fc = 256, feat 80, aux 32
               raw10    RAW 10 bits (1024 classes), rnn = fc = 512
               mol576   MoL, rnn = fc = 576 (the largest the LDS rule takes)
    segments   B = 1, 16, 64, 256;  T = 2000 steps, every step live (stride 21, hop 8)
    widths     1 (= tile), 2, 4, 8 -- a width whose ceil(B / 16) * W workgroups exceed the device's CUs is left out of its row

The timer is `wrnn_timer` around the loop launch (`LoopEngine.last_loop_ms`); the noise is the library's (drawn into the workspace before the timed launch, the
same stream for every width); weights are random-init.  Per (leg, B): one warm-up of each width, then `--reps` timed runs of each, alternating; minimum and
median, us per step, and the ratio tile / width.  Every row also records whether the samples of every width equal tile's bit for bit.

Every (leg, B) runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python scripts/gpu_tile_wide_ab.py --out profiles/tile_wide_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = dict(mol256=dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128),
            raw10=dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=10, feat_dims=80, res_out_dims=128),
            mol576=dict(mode='MOL', rnn_dims=576, fc_dims=576, bits=9, feat_dims=80, res_out_dims=128))
SEGMENTS = (1, 16, 64, 256)
WIDTHS = (1, 2, 4, 8)
T, HOP, STRIDE = 2000, 8, 21
SEED = 0x5EED0123456789AB
KERNELS = {1: 'wrnn_tile_kernel', 2: 'wrnn_tile_wide_kernel', 4: 'wrnn_tile_wide_kernel', 8: 'wrnn_tile_wide_kernel'}
TAG = 'TILE_WIDE_AB '


def one(leg, B, reps):
    """One (leg, B) on the device of this process -> a dict."""
    import numpy as np
    import torch
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.synthetic import random_state_dict
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda', 0)
    g = LEGS[leg]
    sd = random_state_dict(5, compute_dims=8, res_blocks=1, **g)
    eng = LoopEngine(sd, g['mode'], device=dev)
    M, A = g['feat_dims'], g['res_out_dims'] // 4
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    rs = np.random.RandomState(1)
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, M)).astype(np.float32)).to(dev)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 4 * A)).astype(np.float32)).to(dev)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32)
    widths = [W for W in WIDTHS if -(-B // 16) * W <= eng.n_cus]

    def run(W):
        out = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, algo='tile', clusters=W, noise_seed=SEED)
        assert eng.last_loop_kernel() == KERNELS[W], (W, eng.last_loop_kernel())
        return out.clone(), eng.last_loop_ms()

    samples = {W: run(W)[0] for W in widths}       # warm-up
    ms = {W: [] for W in widths}
    for _ in range(reps):
        for W in widths:
            out, t = run(W)
            ms[W].append(t)
            samples[W] = out
    us = lambda v: round(1000.0 * v / T, 3)
    res = dict(leg=leg, B=B, T=T, reps=reps, weight_bytes=eng.weight_bytes, widths=widths,
               us_per_step={str(W): dict(min=us(min(ms[W])), median=us(statistics.median(ms[W]))) for W in widths},
               ratio_min={str(W): round(min(ms[1]) / min(ms[W]), 3) for W in widths if W > 1},
               ratio_median={str(W): round(statistics.median(ms[1]) / statistics.median(ms[W]), 3) for W in widths if W > 1},
               samples_bit_equal_to_tile={str(W): bool(torch.equal(samples[W].view(torch.int32), samples[1].view(torch.int32))) for W in widths if W > 1},
               distinct_samples=int(torch.unique(samples[1]).numel()))
    res['device'] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per (leg, B) child process')
    ap.add_argument('--legs', nargs='*', default=list(LEGS), choices=list(LEGS))
    ap.add_argument('--one', nargs=2, metavar=('LEG', 'B'), help='(a child) run one case and print its JSON line')
    a = ap.parse_args()
    if a.one:
        print(TAG + json.dumps(one(a.one[0], int(a.one[1]), a.reps)), flush=True)
        return
    rows = []
    for leg in a.legs:
        for B in SEGMENTS:
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--one', leg, str(B), '--reps', str(a.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
            if p.returncode != 0 or not line:
                print(p.stdout[-4000:])
                raise SystemExit(f'{leg} B={B}: the child ended with status {p.returncode}; nothing more is started')
            rows.append(json.loads(line[-1][len(TAG):]))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=rows[0]['device'], T=T, hop=HOP, stride=STRIDE, reps=a.reps, legs={k: LEGS[k] for k in a.legs},
               timing='wrnn_timer around the loop launch (LoopEngine.last_loop_ms), the widths alternating on one pack, warm, library noise; us per step = ms / T',
               yardstick='wrnn_tile_kernel (algo tile, width 1) on the same pack; ratio = tile / width',
               rows=[{k: v for k, v in r.items() if k != 'device'} for r in rows])
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
