#!/usr/bin/env python
"""A/B of the WATCHED one-launch loop kernels (`wrnn_generate_segments_watched`: wrnn_generic_kernel and the tile kernels publish how far they have got,
csrc/wrnn_device.h publish_progress) against the parent commit's build, on one MI355X, warm, parent and candidate alternating.

    steps     256 / 256 MoL model, 16 segments, T = 2000 steps, every step live (stride 21, hop 8); legs: tile, tile at width 8, tile_bf16, generic.
              Per repeat one child process per side; a child warms every leg once and times it `--runs` times (`wrnn_timer` around the loop launch,
              `LoopEngine.last_loop_ms`), its figure is the median.  Parent: watch OFF.  Candidate: watch OFF, and watch ON with progress_every = 64.
              Margins: OFF against the parent's own min-max spread over its repeats; ON against the candidate's OFF, twice that spread.
    stream    the same model with hop 128 at 16 kHz, one utterance of 6 s (751 frames, T = 96,128 steps) through `generate_stream(chunk_steps=2200)`:
              wall time to the first chunk and to the last, the number of chunks and a hash of the audio.  Parent: the call runs whole and delivers one
              chunk at the end.  Candidate: live=True.  algo tile, and tile at width 8.

The parent runs from a built checkout of its own (`--baseline-root`: its Python package and its library), the candidate from this tree.  Every child runs
under `timeout`; the first child that fails ends the run.

    python scripts/gpu_live_ab.py --baseline-root <built checkout of the parent commit> --out profiles/live_ab.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'tile': ('tile', 0, 'wrnn_tile_kernel'), 'tile_w8': ('tile', 8, 'wrnn_tile_wide_kernel'), 'tile_bf16': ('tile_bf16', 0, 'wrnn_tile_bf16_kernel'),
        'generic': ('auto', 0, 'wrnn_generic_kernel')}
DIMS = dict(mode='MOL', rnn_dims=256, fc_dims=256, bits=9, feat_dims=80, res_out_dims=128)
B, T, HOP, STRIDE, EVERY = 16, 2000, 8, 21, 64
STREAM_HP = dict(rnn_dims=256, fc_dims=256, bits=9, pad=2, upsample_factors=(4, 4, 8), feat_dims=80, compute_dims=64, res_out_dims=128, res_blocks=3,
                 hop_length=128, sample_rate=16000)
STREAM_FRAMES, CHUNK = 751, 2200
SEED = 0x5EED0123456789AB
TAG = 'LIVE_AB '


def steps(runs, watch):
    """The step legs on the device of this process -> {leg: us per step (median of `runs`)}; watch: also {leg + '_on': ...}."""
    import numpy as np
    import torch
    from wavernn_amd.engine import LoopEngine
    from wavernn_amd.synthetic import random_state_dict
    dev = torch.device('cuda', 0)
    eng = LoopEngine(random_state_dict(5, compute_dims=8, res_blocks=1, **DIMS), DIMS['mode'], device=dev)
    M, A = DIMS['feat_dims'], DIMS['res_out_dims'] // 4
    L = -(-((B - 1) * STRIDE + T) // HOP) * HOP
    rs = np.random.RandomState(1)
    mels_up = torch.from_numpy(rs.uniform(0, 1, (L, M)).astype(np.float32)).to(dev)
    aux = torch.from_numpy(rs.uniform(-1, 1, (L // HOP, 4 * A)).astype(np.float32)).to(dev)
    seg_pos, seg_lim = np.arange(B, dtype=np.int32) * STRIDE, np.full(B, L, np.int32)
    res, ref = {}, {}
    for on in ((False, True) if watch else (False,)):
        for leg, (algo, width, kernel) in LEGS.items():
            kw = {}
            if on:
                kw['watch'] = (torch.zeros(eng.watch_words(B, T, algo=algo, clusters=width), dtype=torch.int32, device=dev), EVERY)
            ms = []
            for i in range(runs + 1):       # the first run warms
                out = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, HOP, algo=algo, clusters=width, noise_seed=SEED, **kw)
                assert eng.last_loop_kernel() == kernel, eng.last_loop_kernel()
                if i:
                    ms.append(eng.last_loop_ms())
            if on:
                assert torch.equal(out, ref[leg]) and int(kw['watch'][0].min()) == T
            ref.setdefault(leg, out.clone())
            res[leg + ('_on' if on else '')] = round(1000.0 * statistics.median(ms) / T, 3)
    res['device'] = torch.cuda.get_device_name(0)
    return res


def stream(width, live):
    """One 6 s utterance through generate_stream -> first-chunk and total wall time (the second of two calls: the first warms)."""
    import warnings
    import numpy as np
    import torch
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel, random_state_dict
    dev = torch.device('cuda', 0)
    sd = random_state_dict(71, mode='MOL', **STREAM_HP)
    model = WaveRNN(**STREAM_HP, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    model = model.to(dev)
    model.loop_algo, model.tile_width, model.noise_source, model.noise_seed = 'tile', width, 'library', 977
    mel = torch.tensor(random_mel(72, STREAM_FRAMES, n_mels=80)).unsqueeze(0)
    kw = dict(live=True) if live else {}
    res = {}
    for frames in (40, STREAM_FRAMES):      # a short call warms everything
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0, first, chunks = time.perf_counter(), None, []
            for c in model.generate_stream(mel[..., :frames], False, chunk_steps=CHUNK, **kw):
                first = first if first is not None else time.perf_counter() - t0
                chunks.append(c)
            total = time.perf_counter() - t0
        audio = np.concatenate(chunks)
        res = dict(first_chunk_ms=round(first * 1e3, 1), total_ms=round(total * 1e3, 1), chunks=len(chunks), samples=int(audio.shape[0]),
                   loop_ms=round(float(model.last_loop_ms), 1), kernel=model.last_loop_kernel, sha256=hashlib.sha256(audio.tobytes()).hexdigest()[:16])
    return res


def child(root, args, limit):
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--root', root] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
    if p.returncode != 0 or not line:
        print(p.stdout[-4000:])
        raise SystemExit(f'{args} under {root}: the child ended with status {p.returncode}; nothing more is started')
    return json.loads(line[-1][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline-root', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3, help='timed runs per leg in a child')
    ap.add_argument('--no-stream', action='store_true')
    ap.add_argument('--root', default=ROOT, help='(a child) the tree to import wavernn_amd from')
    ap.add_argument('--steps', choices=['off', 'watch'], help='(a child) the step legs')
    ap.add_argument('--stream', nargs=2, metavar=('WIDTH', 'LIVE'), help='(a child) the 6 s utterance')
    a = ap.parse_args()
    if a.steps or a.stream:
        sys.path.insert(0, os.path.abspath(a.root))
        import torch
        assert torch.cuda.is_available(), 'needs a HIP device'
        res = steps(a.runs, a.steps == 'watch') if a.steps else stream(int(a.stream[0]), a.stream[1] == '1')
        print(TAG + json.dumps(res), flush=True)
        return
    if not a.baseline_root:
        ap.error('--baseline-root: a built checkout of the parent commit')
    parent, cand = [], []
    for _ in range(a.reps):
        parent.append(child(a.baseline_root, ['--steps', 'off', '--runs', str(a.runs)], 240))
        cand.append(child(ROOT, ['--steps', 'watch', '--runs', str(a.runs)], 240))
        print(json.dumps(dict(parent=parent[-1], candidate=cand[-1])), flush=True)
    rows = {}
    for leg in LEGS:
        p, c, on = [r[leg] for r in parent], [r[leg] for r in cand], [r[leg + '_on'] for r in cand]
        spread = round(max(p) - min(p), 3)
        rows[leg] = dict(parent_us=p, candidate_off_us=c, candidate_on_us=on, parent_spread_us=spread,
                         off_median_minus_parent_median_us=round(statistics.median(c) - statistics.median(p), 3),
                         off_within_parent_min_max=bool(min(p) <= statistics.median(c) <= max(p)),
                         on_median_minus_off_median_us=round(statistics.median(on) - statistics.median(c), 3),
                         on_within_twice_the_spread=bool(statistics.median(on) - statistics.median(c) <= 2 * spread))
    res = dict(device=cand[0]['device'], segments=B, T=T, every=EVERY, reps=a.reps, runs=a.runs, dims=DIMS,
               timing='wrnn_timer around the loop launch (LoopEngine.last_loop_ms); one child process per side and repeat, alternating; us per step = '
                      'median of the runs / T', steps=rows)
    if not a.no_stream:
        res['stream'] = dict(hparams={k: v for k, v in STREAM_HP.items()}, frames=STREAM_FRAMES, chunk_steps=CHUNK, rows={})
        for width in (0, 8):
            p, c = child(a.baseline_root, ['--stream', str(width), '0'], 420), child(ROOT, ['--stream', str(width), '1'], 420)
            res['stream']['rows'][f'tile_width_{width}'] = dict(parent=p, candidate_live=c, same_audio=p['sha256'] == c['sha256'],
                                                                first_chunk_before_the_parents_only_one=c['first_chunk_ms'] < p['first_chunk_ms'])
            print(json.dumps(res['stream']['rows'][f'tile_width_{width}']), flush=True)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
