#!/usr/bin/env python
"""A/B of the two loop kernels that run a PRUNED generic pack, on one MI355X, one build and one pack per leg: `wrnn_tile_sparse_kernel` (algo 'tile_sparse':
the surviving 16x1 blocks only, csrc/wrnn_tile_sparse.hip) against `wrnn_tile_kernel` (algo 'tile': the masked weights dense, csrc/wrnn_tile.hip -- what a
caller could run for such a model before, the yardstick).  After scripts/gpu_tile_ab.py.

    legs       mol256_gf   MoL, rnn = fc = 256, feat 80, aux 32, 95 % of the 16x1 blocks pruned in the GRU matrices and in fc1 / fc2
               mol256_g    the same, GRU matrices only (dense fc stages beside sparse GRU stages)
               raw10_gf    RAW 10 bits (1024 classes), rnn = fc = 512, 95 % GRU + fc
               mol576_gf   MoL, rnn = fc = 576 (the largest the LDS rule takes), 95 % GRU + fc
               mol256_50   mol256_gf at 50 %
               mol256_60 / 70 / 75 / 80 / 90   ... and at the levels between, 256 segments only: where the admission threshold of the view belongs
    segments   B = 64, 256, 1024;  T = 2000 steps, every step live (stride 21, hop 8)

The timer is `wrnn_timer` around the loop launch (`LoopEngine.last_loop_ms`); the noise is the library's (drawn into the workspace before the timed launch, the
same stream for both kernels); weights are random-init, pruned with `prune.block_prune_state_dict`.  Per (leg, B): one warm-up of each kernel, then `--reps`
timed runs of each, alternating; minimum and median, us per step, and the ratio tile / tile_sparse.  The samples of the two kernels are compared (RAW: how many
differ; MoL: max abs difference; both: whether every bit is equal), and at B = 64 the teacher-forced logits too (fed `tile`'s samples): reported, not asserted.

Every (leg, B) runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python scripts/gpu_tile_sparse_ab.py --out profiles/tile_sparse_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MOL256 = dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128)
LEGS = dict(mol256_gf=dict(MOL256, sparsity=0.95, linear=True),
            mol256_g=dict(MOL256, sparsity=0.95, linear=False),
            raw10_gf=dict(mode='RAW', rnn_dims=512, fc_dims=512, bits=10, feat_dims=80, res_out_dims=128, sparsity=0.95, linear=True),
            mol576_gf=dict(mode='MOL', rnn_dims=576, fc_dims=576, bits=9, feat_dims=80, res_out_dims=128, sparsity=0.95, linear=True),
            mol256_50=dict(MOL256, sparsity=0.50, linear=True),
            # ... and the levels between, at 256 segments: where the admission threshold belongs
            mol256_60=dict(MOL256, sparsity=0.60, linear=True, segments=(256,)), mol256_70=dict(MOL256, sparsity=0.70, linear=True, segments=(256,)),
            mol256_75=dict(MOL256, sparsity=0.75, linear=True, segments=(256,)), mol256_80=dict(MOL256, sparsity=0.80, linear=True, segments=(256,)),
            mol256_90=dict(MOL256, sparsity=0.90, linear=True, segments=(256,)))
SEGMENTS = (64, 256, 1024)
T, HOP, STRIDE = 2000, 8, 21
SEED = 0x5EED0123456789AB
KERNELS = dict(tile='wrnn_tile_kernel', tile_sparse='wrnn_tile_sparse_kernel')


def one(leg, B, reps):
    """One (leg, B) on the device of this process -> a dict."""
    import warnings
    import numpy as np
    import torch
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.prune import block_prune_state_dict
    from wavernn_amd.synthetic import random_state_dict
    assert torch.cuda.is_available(), 'needs a HIP device'
    dev = torch.device('cuda', 0)
    g = LEGS[leg]
    hp = {k: g[k] for k in ('mode', 'rnn_dims', 'fc_dims', 'bits', 'feat_dims', 'res_out_dims')}
    sd, _ = block_prune_state_dict(random_state_dict(5, compute_dims=8, res_blocks=1, **hp), g['sparsity'], linear=g['linear'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        eng = LoopEngine(sd, g['mode'], device=dev)
    view, kept, total = eng.tile_sparse_view()
    if view == 0:               # below the admission threshold: what the planner answers is the result of this leg
        from wavernn_amd import _lib
        try:
            eng.plan(B, T, algo='tile_sparse')
            raise AssertionError('a pack without a view was planned')
        except _lib.WrnnError as e:
            return dict(leg=leg, B=B, view=0, blocks_kept=kept, blocks_total=total, refused=str(e), device=torch.cuda.get_device_name(0))
    assert view == (2 if g['linear'] else 1), (leg, view, kept, total)
    M, A = g['feat_dims'], g['res_out_dims'] // 4
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    rs = np.random.RandomState(1)
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, M)).astype(np.float32)).to(dev)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 4 * A)).astype(np.float32)).to(dev)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32)

    def run(algo, **kw):
        out = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, algo=algo, noise_seed=SEED, **kw)
        assert eng.last_loop_kernel() == KERNELS[algo], (algo, eng.last_loop_kernel())
        return out, eng.last_loop_ms()

    outs = {algo: run(algo)[0].cpu().numpy() for algo in KERNELS}          # warm-up, and the samples
    ms = {algo: [] for algo in KERNELS}
    for _ in range(reps):
        for algo in KERNELS:
            ms[algo].append(run(algo)[1])
    us = lambda v: round(1000.0 * v / T, 3)
    res = dict(leg=leg, B=B, T=T, reps=reps, view=view, blocks_kept=kept, blocks_total=total,
               tile_us_per_step=dict(min=us(min(ms['tile'])), median=us(statistics.median(ms['tile']))),
               tile_sparse_us_per_step=dict(min=us(min(ms['tile_sparse'])), median=us(statistics.median(ms['tile_sparse']))),
               speedup_min=round(min(ms['tile']) / min(ms['tile_sparse']), 3),
               speedup_median=round(statistics.median(ms['tile']) / statistics.median(ms['tile_sparse']), 3),
               samples_bit_identical=bool(np.array_equal(outs['tile'].view(np.uint32), outs['tile_sparse'].view(np.uint32))))
    if g['mode'] == 'MOL':
        res['samples_max_abs_diff'] = float(np.abs(outs['tile_sparse'] - outs['tile']).max())
    else:
        res['samples_differing'] = int(np.count_nonzero(outs['tile_sparse'] != outs['tile']))
        res['samples'] = int(outs['tile'].size)
    if B == LEGS[leg].get('segments', SEGMENTS)[0]:        # the observation: teacher-forced with `tile`'s samples, are the logits of the two kernels the same bits?
        fed = torch.from_numpy(outs['tile']).to(dev)
        lg = {algo: run(algo, force_x=fed, want_logits=True)[0][1].cpu().numpy() for algo in KERNELS}
        res['forced_logits_bit_identical'] = bool(np.array_equal(lg['tile'].view(np.uint32), lg['tile_sparse'].view(np.uint32)))
        res['forced_logits_max_abs_diff'] = float(np.abs(lg['tile'] - lg['tile_sparse']).max())
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
        print('TILE_SPARSE_AB ' + json.dumps(one(a.one[0], int(a.one[1]), a.reps)), flush=True)
        return
    rows = []
    for leg in a.legs:
        for B in LEGS[leg].get('segments', SEGMENTS):
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--one', leg, str(B), '--reps', str(a.reps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('TILE_SPARSE_AB ')]
            if p.returncode != 0 or not line:
                print(p.stdout[-4000:])
                raise SystemExit(f'{leg} B={B}: the child ended with status {p.returncode}; nothing more is started')
            rows.append(json.loads(line[-1][len('TILE_SPARSE_AB '):]))
            print(json.dumps(rows[-1]), flush=True)
    res = dict(device=rows[0]['device'], T=T, hop=HOP, stride=STRIDE, reps=a.reps, legs={k: LEGS[k] for k in a.legs},
               timing='wrnn_timer around the loop launch (LoopEngine.last_loop_ms), the two kernels alternating on one pack, warm, library noise; us per step = ms / T',
               yardstick='wrnn_tile_kernel (algo tile) on the masked dense weights of the same pack; speedup = tile / tile_sparse',
               rows=[{k: v for k, v in r.items() if k != 'device'} for r in rows])
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
