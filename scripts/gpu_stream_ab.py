#!/usr/bin/env python
"""A/B of unbatched synthesis of a LIST of utterances on one MI355X: 16 MoL utterances of 2-6 s (random-init weights of the shipped dims: no
trained checkpoint ships with the repository; random mels), 'library' noise, the same seeds on every path.

    (a) serial    16 back-to-back `WaveRNN.generate(batched=False)` calls -- the only way before `generate_unbatched` (each writes its WAV, as it must)
    (b) list      one `batch.generate_unbatched` call: 16 unfolded segments of one loop call
    (c) streamed  the same with chunk_steps=2200: `wrnn_post_chunk` + a copy behind every slice

and, for one 6 s utterance, `first_chunk_ms` of `WaveRNN.generate_stream` (chunk_steps=2200) against the wall time of `generate(batched=False)`.
One process, warm (one untimed pass of every contender), the contenders alternating, five repeats, minimum and median; host clock around calls that
return finished audio on the host.  The protocol of scripts/gpu_taco_batch_ab.py.

    python scripts/gpu_stream_ab.py --out profiles/stream_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
#: frames per utterance: 2.0 .. 6.0 s at 22,050 Hz and hop 275 (161 .. 481 frames), in no particular order
FRAMES = (321, 161, 481, 241, 402, 187, 449, 280, 214, 361, 172, 430, 301, 255, 467, 199)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk-steps', type=int, default=2200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import SHIPPED, random_mel, random_state_dict
    dev = torch.device('cuda', 0)
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(61, mode='MOL').items()}, strict=True)
    model = model.to(dev)
    model.noise_source = 'library'
    hop, rate = model.hop_length, model.sample_rate
    mels = [torch.from_numpy(random_mel(5000 + k, f)).unsqueeze(0).to(dev) for k, f in enumerate(FRAMES)]
    seeds = [900 + k for k in range(len(mels))]
    tmp = tempfile.mkdtemp()
    kernels = {}

    def serial():
        outs = []
        for u, m in enumerate(mels):
            model.noise_seed = seeds[u]
            outs.append(model.generate(m, os.path.join(tmp, f'{u}.wav'), False, 11000, 550, True))
        kernels['serial'] = model.last_loop_kernel
        return outs

    def as_list(chunk_steps=None, tm=None):
        outs = generate_unbatched(model, mels, True, seeds, chunk_steps=chunk_steps, timings=tm)
        kernels['streamed' if chunk_steps else 'list'] = model.last_loop_kernel
        return outs

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    # warm, and the three paths give the same audio
    ra, rb, rc = serial(), as_list(), as_list(a.chunk_steps)
    same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(ra, rb, rc))
    ts = dict(serial=[], list=[], streamed=[])
    loop_ms, first_ms = dict(list=[], streamed=[]), []
    for _ in range(a.reps):
        ts['serial'].append(wall(serial)[0])
        tm = {}
        ts['list'].append(wall(lambda: as_list(None, tm))[0])
        loop_ms['list'].append(tm['loop_ms'])
        tm = {}
        ts['streamed'].append(wall(lambda: as_list(a.chunk_steps, tm))[0])
        loop_ms['streamed'].append(tm['loop_ms'])
        first_ms.append(tm['first_chunk_ms'])
        slices = tm['slices']

    # one 6 s utterance: the first chunk of generate_stream against the whole generate()
    long_mel = mels[FRAMES.index(max(FRAMES))]
    model.noise_seed = 977
    whole = model.generate(long_mel, os.path.join(tmp, 'long.wav'), False, 11000, 550, True)
    assert np.array_equal(np.concatenate(list(model.generate_stream(long_mel, True, chunk_steps=a.chunk_steps))), whole)
    one = dict(generate=[], stream_first=[], stream_total=[])
    for _ in range(a.reps):
        one['generate'].append(wall(lambda: model.generate(long_mel, os.path.join(tmp, 'long.wav'), False, 11000, 550, True))[0])
        torch.cuda.synchronize()
        t0, first = time.perf_counter(), None
        for _c in model.generate_stream(long_mel, True, chunk_steps=a.chunk_steps):
            first = first if first is not None else (time.perf_counter() - t0) * 1e3
        one['stream_total'].append((time.perf_counter() - t0) * 1e3)
        one['stream_first'].append(first)

    f = lambda v: dict(min_ms=round(min(v), 3), median_ms=round(statistics.median(v), 3), max_ms=round(max(v), 3))
    steps = [n * hop for n in FRAMES]
    res = dict(device=torch.cuda.get_device_name(0), frames=list(FRAMES), seconds=[round(n * hop / rate, 2) for n in FRAMES], reps=a.reps,
               chunk_steps=a.chunk_steps, weights='random init, shipped dims, MOL', noise='library',
               timing='host clock around calls that return finished audio on the host, one process, warm, contenders alternating; ms',
               kernels=kernels, same_audio_on_all_three=bool(same), sum_steps=sum(steps), max_steps=max(steps), sum_over_max=round(sum(steps) / max(steps), 3),
               serial=f(ts['serial']), list=f(ts['list']), streamed=f(ts['streamed']),
               list_loop_ms=f(loop_ms['list']), streamed_loop_ms=f(loop_ms['streamed']), streamed_first_chunk_ms=f(first_ms), streamed_slices=slices,
               us_per_step=dict(serial_min=round(min(ts['serial']) * 1e3 / sum(steps), 3), list_loop_min=round(min(loop_ms['list']) * 1e3 / max(steps), 3),
                                streamed_loop_min=round(min(loop_ms['streamed']) * 1e3 / max(steps), 3)),
               serial_over_list_min=round(min(ts['serial']) / min(ts['list']), 3), serial_over_list_median=round(statistics.median(ts['serial']) / statistics.median(ts['list']), 3),
               streamed_over_list_min=round(min(ts['streamed']) / min(ts['list']), 4),
               streamed_over_list_median=round(statistics.median(ts['streamed']) / statistics.median(ts['list']), 4),
               # the claim: the list call beats the serial calls by more than the spread of the repeats -- its slowest repeat under their fastest
               list_slowest_under_serial_fastest=bool(max(ts['list']) < min(ts['serial'])),
               one_utterance=dict(frames=max(FRAMES), seconds=round(max(FRAMES) * hop / rate, 2), generate_wall=f(one['generate']),
                                  stream_first_chunk=f(one['stream_first']), stream_total=f(one['stream_total']),
                                  first_chunk_audio_ms=round(a.chunk_steps / rate * 1e3, 1)))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
