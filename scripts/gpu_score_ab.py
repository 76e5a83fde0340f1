#!/usr/bin/env python
"""What scoring costs on one MI355X, and what the path a user has today costs on the same card.  A measurement: nothing is asserted but that both paths
give the same corpus mean.

    loss      `wrnn_nll` alone on [12100][256][30] (MOL) and [12100][16][512] (RAW) logits: HIP events around each of `--reps` launches after two
              warm-up launches; bytes read (logits + targets) over that time, as a fraction of the 6.29 TB/s achievable HBM rate
    corpus    `score_corpus` on 16 and on 256 utterances of 2 s (160 frames = 44,000 steps, MOL, random-init weights): the loop (wrnn_timer), the loss
              (events) and the wall time of the call (host clock around a call that ends in a synchronise), against `WaveRNN.forward` of model.py as
              PyTorch-ROCm ops (nn.GRU) with a torch restatement of the loss, in micro-batches of `--torch-batch` utterances (every intermediate of the
              forward is a [B, 44000, 512] tensor)

Every part runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python scripts/gpu_score_ab.py --out profiles/score_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.29e12
FRAMES, HOP = 160, 275
LOSS_SHAPES = dict(mol=('MOL', 12100, 256, 30), raw=('RAW', 12100, 16, 512))


def stats(ms):
    return dict(min=round(min(ms), 4), median=round(statistics.median(ms), 4), n=len(ms))


def loss_alone(which, reps):
    import numpy as np
    import torch
    from wavernn_amd import _lib
    from wavernn_amd.score import nll_on_device
    mode, T, n, C = LOSS_SHAPES[which]
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.randn(T, n, C, generator=g, device=dev) * (3.0 if mode == 'MOL' else 4.0)
    lab = torch.randint(0, 65536 if mode == 'MOL' else C, (n, T), generator=g, device=dev)
    x = (2 * lab.float() / (65535 if mode == 'MOL' else C - 1) - 1).contiguous()
    if mode == 'MOL':
        logits[..., 10:20] = x.t()[..., None] + 0.01 * logits[..., 10:20]
        logits[..., 20:] = -4 + logits[..., 20:] * 0.5
    lens = torch.full((n,), T, dtype=torch.int32, device=dev)
    L = _lib.lib()
    res = {}
    for per_step in (True, False):
        for _ in range(2):
            nll_on_device(L, 0, mode, logits, x, lens, per_step)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _, total = nll_on_device(L, 0, mode, logits, x, lens, per_step)
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        read = T * n * (C + 1) * 4
        res['with_per_step' if per_step else 'sums_only'] = dict(
            us=stats([1000 * m for m in ms]), bytes_read=read, tb_per_s_at_min=round(read / (min(ms) * 1e-3) / 1e12, 3),
            fraction_of_hbm_rate_at_min=round(read / (min(ms) * 1e-3) / HBM_BYTES_PER_S, 4),
            fraction_of_hbm_rate_at_median=round(read / (statistics.median(ms) * 1e-3) / HBM_BYTES_PER_S, 4))
    assert np.isfinite(total.cpu().numpy()).all()
    return dict(part='loss', mode=mode, shape=[T, n, C], workgroups=n, mean_nll=float(total.sum().item() / (T * n)), **res)


def corpus_inputs(n):
    import numpy as np
    import torch
    from wavernn_amd.synthetic import random_mel
    mels = [torch.from_numpy(random_mel(500 + u, FRAMES)).unsqueeze(0) for u in range(n)]
    t = np.arange(FRAMES * HOP)
    wavs = [np.clip(0.6 * np.sin(t * (0.03 + 0.0002 * u)) + 0.05 * np.random.RandomState(u).standard_normal(t.size), -1, 1).astype(np.float32)
            for u in range(n)]
    return mels, wavs


def make_model():
    import numpy as np
    import torch
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_state_dict, SHIPPED
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(12, mode='MOL').items()}, strict=True)
    return model.to('cuda')


def corpus_hip(n, reps):
    import torch
    from wavernn_amd.batch import score_corpus
    model = make_model()
    mels, wavs = corpus_inputs(n)
    rows = []
    for i in range(reps + 1):              # the first call is the warm-up (packs, workspaces, code objects)
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = score_corpus(model, mels, wavs, timings=tm)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if i:
            rows.append((tm['loop_ms'], tm['loss_ms'], wall))
        print(f'score_corpus n={n} call {i}: loop {tm["loop_ms"]:.1f} ms, loss {tm["loss_ms"]:.3f} ms, wall {wall:.1f} ms', flush=True)
    mean = sum(r['nll_sum'] for r in res) / sum(r['steps'] for r in res)
    return dict(part='corpus_hip', utterances=n, steps=FRAMES * HOP, kernel=model.last_loop_kernel, nll_mean=mean,
                loop_ms=stats([r[0] for r in rows]), loss_ms=stats([r[1] for r in rows]), wall_ms=stats([r[2] for r in rows]))


def torch_mol_nll(y_hat, y):
    """The MoL loss as torch ops (utils/distribution.py:16-84 restated): y_hat [B, T, 30], y [B, T] -> [B, T]."""
    import math
    import torch
    import torch.nn.functional as F
    mix, mean, ls = y_hat[..., :10], y_hat[..., 10:20], y_hat[..., 20:].clamp(min=math.log(1e-14))
    y = y.unsqueeze(-1)
    inv, cy, half = torch.exp(-ls), y - mean, 1.0 / 65535
    hi, lo, mid = inv * (cy + half), inv * (cy - half), inv * cy
    delta = torch.sigmoid(hi) - torch.sigmoid(lo)
    inner = torch.where(delta > 1e-5, torch.log(delta.clamp(min=1e-12)), mid - ls - 2 * F.softplus(mid) - math.log(65535 / 2))
    lp = torch.where(y < -0.999, hi - F.softplus(hi), torch.where(y > 0.999, -F.softplus(lo), inner)) + F.log_softmax(mix, -1)
    return -torch.logsumexp(lp, -1)


def corpus_torch(n, reps, batch):
    import numpy as np
    import torch
    from wavernn_amd import fold
    from wavernn_amd.score import prepare_targets
    model = make_model().eval()
    mels, wavs = corpus_inputs(n)
    y = torch.from_numpy(np.stack([prepare_targets(w, 'MOL')[1] for w in wavs])).cuda()
    x = torch.cat([torch.zeros(n, 1, device='cuda'), y[:, :-1]], dim=1)
    m = fold.pad_tensor(torch.cat(mels).cuda().transpose(1, 2), pad=model.pad, side='both').transpose(1, 2)
    rows = []
    for i in range(reps + 1):
        fwd = loss = 0.0
        total = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for b0 in range(0, n, batch):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                y_hat = model(x[b0:b0 + batch], m[b0:b0 + batch])
                ev[1].record()
                total += float(torch_mol_nll(y_hat, y[b0:b0 + batch]).double().sum().item())
                ev[2].record()
                torch.cuda.synchronize()
                fwd += ev[0].elapsed_time(ev[1])
                loss += ev[1].elapsed_time(ev[2])
                del y_hat
        wall = (time.perf_counter() - t0) * 1e3
        if i:
            rows.append((fwd, loss, wall))
        print(f'torch forward n={n} call {i}: forward {fwd:.1f} ms, loss {loss:.1f} ms, wall {wall:.1f} ms', flush=True)
    return dict(part='corpus_torch', utterances=n, steps=FRAMES * HOP, micro_batch=batch, nll_mean=total / (n * FRAMES * HOP),
                forward_ms=stats([r[0] for r in rows]), loss_ms=stats([r[1] for r in rows]), wall_ms=stats([r[2] for r in rows]),
                peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10, help='timed wrnn_nll launches')
    ap.add_argument('--corpus-reps', type=int, default=2, help='timed calls of each corpus path (after one warm-up call)')
    ap.add_argument('--torch-batch', type=int, default=16)
    ap.add_argument('--timeout', type=int, default=280, help='seconds per child process')
    ap.add_argument('--one', nargs=2, metavar=('PART', 'ARG'), help='(a child) run one part and print its JSON line')
    a = ap.parse_args()
    if a.one:
        import torch
        assert torch.cuda.is_available(), 'needs a HIP device'
        part, arg = a.one
        res = (loss_alone(arg, a.reps) if part == 'loss' else corpus_hip(int(arg), a.corpus_reps) if part == 'corpus_hip'
               else corpus_torch(int(arg), a.corpus_reps, a.torch_batch))
        res['device'] = torch.cuda.get_device_name(0)
        print('SCORE_AB ' + json.dumps(res), flush=True)
        return
    rows = []
    for part, arg in (('loss', 'mol'), ('loss', 'raw'), ('corpus_hip', '16'), ('corpus_torch', '16'), ('corpus_hip', '256'), ('corpus_torch', '256')):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--one', part, arg, '--reps', str(a.reps),
               '--corpus-reps', str(a.corpus_reps), '--torch-batch', str(a.torch_batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('SCORE_AB ')]
        if p.returncode != 0 or not line:
            print(p.stdout[-4000:])
            raise SystemExit(f'{part} {arg}: the child ended with status {p.returncode}; nothing more is started')
        rows.append(json.loads(line[-1][len('SCORE_AB '):]))
        print(json.dumps(rows[-1]), flush=True)
    hip = {r['utterances']: r for r in rows if r['part'] == 'corpus_hip'}
    tor = {r['utterances']: r for r in rows if r['part'] == 'corpus_torch'}
    summary = [dict(utterances=n, hip_wall_ms=hip[n]['wall_ms']['median'], torch_wall_ms=tor[n]['wall_ms']['median'],
                    torch_over_hip=round(tor[n]['wall_ms']['median'] / hip[n]['wall_ms']['median'], 3),
                    nll_mean_difference=abs(hip[n]['nll_mean'] - tor[n]['nll_mean'])) for n in sorted(hip)]
    res = dict(device=rows[0]['device'], hbm_bytes_per_s=HBM_BYTES_PER_S,
               timing='loss: HIP events around one wrnn_nll launch, warm; corpus: wrnn_timer (loop), events (loss), host clock around the synchronised call (wall); '
                      'one warm-up call of each corpus path is not counted',
               rows=[{k: v for k, v in r.items() if k != 'device'} for r in rows], summary=summary)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
