#!/usr/bin/env python
"""A/B of `wrnn_tile_bf16_kernel` (algo 'tile_bf16': the eight loop matrices in bfloat16 on v_mfma_f32_16x16x32_bf16, csrc/wrnn_tile_bf16.hip) against
`wrnn_tile_kernel` (algo 'tile': float32 weights on v_mfma_f32_16x16x4_f32, csrc/wrnn_tile.hip -- the yardstick), on one MI355X, one build and one pack per
leg.  After scripts/gpu_tile_sparse_ab.py.

    legs       mol256   MoL, rnn = fc = 256, feat 80, aux 32
               raw10    RAW 10 bits (1024 classes), rnn = fc = 512
               mol576   MoL, rnn = fc = 576 (the largest the LDS rule takes)
    segments   B = 64, 256, 1024;  T = 2000 steps, every step live (stride 21, hop 8)

The timer is `wrnn_timer` around the loop launch (`LoopEngine.last_loop_ms`); the noise is the library's (drawn into the workspace before the timed launch, the
same stream for both kernels); weights are random-init.  Per (leg, B): one warm-up of each kernel, then `--reps` timed runs of each, alternating; minimum and
median, us per step, and the ratio tile / tile_bf16.  The two kernels run DIFFERENT models (float32 and rounded weights), so their samples are not compared;
what each row records of the arithmetic is max |logits(tile_bf16) - logits(tile on a pack of the ROUNDED weights)| over the first 64 steps, both teacher-forced
with the same samples: the two kernels on the same weights.  Reported, not asserted.

Every (leg, B) runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python scripts/gpu_tile_bf16_ab.py --out profiles/tile_bf16_ab.json
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
SEGMENTS = (64, 256, 1024)
T, T_LOGITS, HOP, STRIDE = 2000, 64, 8, 21
SEED = 0x5EED0123456789AB
KERNELS = dict(tile='wrnn_tile_kernel', tile_bf16='wrnn_tile_bf16_kernel')
TAG = 'TILE_BF16_AB '


def one(leg, B, reps):
    """One (leg, B) on the device of this process -> a dict."""
    import numpy as np
    import torch
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.synthetic import bf16_round_state_dict, random_state_dict
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda', 0)
    g = LEGS[leg]
    sd = random_state_dict(5, compute_dims=8, res_blocks=1, **g)
    eng = LoopEngine(sd, g['mode'], device=dev)
    assert eng.tile_bf16_bytes() > 0
    M, A = g['feat_dims'], g['res_out_dims'] // 4
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    rs = np.random.RandomState(1)
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, M)).astype(np.float32)).to(dev)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 4 * A)).astype(np.float32)).to(dev)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32)

    def run(e, algo, steps=T, **kw):
        out = e.run_segments(mels_up, aux, seg_pos, seg_lim, steps, None, HOP, algo=algo, noise_seed=SEED, **kw)
        assert e.last_loop_kernel() == KERNELS[algo], (algo, e.last_loop_kernel())
        return out, e.last_loop_ms()

    for algo in KERNELS:                            # warm-up
        run(eng, algo)
    ms = {algo: [] for algo in KERNELS}
    for _ in range(reps):
        for algo in KERNELS:
            ms[algo].append(run(eng, algo)[1])
    us = lambda v: round(1000.0 * v / T, 3)
    res = dict(leg=leg, B=B, T=T, reps=reps, weight_bytes=eng.weight_bytes, bf16_view_bytes=eng.tile_bf16_bytes(),
               tile_us_per_step=dict(min=us(min(ms['tile'])), median=us(statistics.median(ms['tile']))),
               tile_bf16_us_per_step=dict(min=us(min(ms['tile_bf16'])), median=us(statistics.median(ms['tile_bf16']))),
               ratio_min=round(min(ms['tile']) / min(ms['tile_bf16']), 3),
               ratio_median=round(statistics.median(ms['tile']) / statistics.median(ms['tile_bf16']), 3))
    # the two kernels on the same weights: a second pack, of the rounded weights, run by `tile`; both fed its samples
    eng_q = LoopEngine(bf16_round_state_dict(sd), g['mode'], device=dev)
    fed = run(eng_q, 'tile', T_LOGITS)[0]
    lg_t = run(eng_q, 'tile', T_LOGITS, force_x=fed, want_logits=True)[0][1]
    lg_b = run(eng, 'tile_bf16', T_LOGITS, force_x=fed, want_logits=True)[0][1]
    res['forced_logits_steps'] = T_LOGITS
    res['forced_logits_max_abs_diff'] = float((lg_t - lg_b).abs().max())
    res['forced_logits_max_abs'] = float(lg_t.abs().max())
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
               timing='wrnn_timer around the loop launch (LoopEngine.last_loop_ms), the two kernels alternating on one pack, warm, library noise; us per step = ms / T',
               yardstick='wrnn_tile_kernel (algo tile) on the float32 weights of the same pack; ratio = tile / tile_bf16',
               rows=[{k: v for k, v in r.items() if k != 'device'} for r in rows])
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
