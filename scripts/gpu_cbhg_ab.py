#!/usr/bin/env python
"""A/B of Tacotron's encoder and post-net on one MI355X: the torch-op path (what `generate(kernel=True)` runs: MIOpen / rocBLAS ops +
`wrnn_bigru`) against the HIP path (`cbhg_kernel=True`: `wrnn_taco_encode` / `wrnn_taco_postnet`, csrc/wrnn_cbhg.hip).  One process, warm,
HIP events, the two paths alternating; plus the FIRST call of each path at a length the process has not seen (MIOpen's per-shape
set-up shows there).  Random-init weights of the reference's architecture (tests/golden/tacotron_shapes.json).

    python scripts/gpu_cbhg_ab.py --out profiles/<tag>_cbhg_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IDS_TEXT = 'Scientists at the CERN laboratory say they have discovered a new particle.'


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(torch_fn, hip_fn, reps, warm=3):
    for _ in range(warm):
        torch_fn()
        hip_fn()
    torch.cuda.synchronize()
    t, h = [], []
    for _ in range(reps):
        t.append(event_ms(torch_fn))
        h.append(event_ms(hip_fn))
    s = lambda v: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    return dict(torch=s(t), hip=s(h), reps=reps, speedup_median=round(statistics.median(t) / statistics.median(h), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    dev = torch.device('cuda', 0)
    shapes = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device=dev)
    tts._bigru_kernel = True                                     # the torch-op path of generate(kernel=True)
    ids = text_to_ids(IDS_TEXT)
    g = torch.Generator().manual_seed(7)
    mels = {n: (0.5 * torch.randn(1, 80, n, generator=g)).to(dev) for n in (200, 800, 333)}

    def post_torch(m):
        return F.linear(tts._cbhg(m, 'postnet', tts._post_k), tts.p['post_proj.weight'])

    res = dict(device=torch.cuda.get_device_name(0), timing='HIP events around one call, torch / hip alternating, warm; ms',
               note='encode = embedding + pre-net + encoder CBHG + GRU + encoder_proj; postnet = post-net CBHG + GRU + post_proj')
    with torch.no_grad():
        tts.encode_kernel(ids)                                   # creates the wrnn_taco_front (not timed)
        res['encode_74_chars'] = ab(lambda: tts.encode(ids), lambda: tts.encode_kernel(ids), a.reps)
        for n in (200, 800):
            res[f'postnet_{n}_frames'] = ab(lambda: post_torch(mels[n]), lambda: tts.postnet_kernel(mels[n]), a.reps)
        # first call at a length this process has not run (host clock around the call and a synchronise), then the second call
        unseen_ids = ids[:61]
        first = {}
        first['encode_61_chars'] = dict(torch_first_ms=round(wall_ms(lambda: tts.encode(unseen_ids)), 3),
                                        torch_second_ms=round(wall_ms(lambda: tts.encode(unseen_ids)), 3))
        unseen_ids = ids[:53]
        first['encode_53_chars'] = dict(hip_first_ms=round(wall_ms(lambda: tts.encode_kernel(unseen_ids)), 3),
                                        hip_second_ms=round(wall_ms(lambda: tts.encode_kernel(unseen_ids)), 3),
                                        torch_first_ms=round(wall_ms(lambda: tts.encode(unseen_ids)), 3))
        first['postnet_333_frames'] = dict(hip_first_ms=round(wall_ms(lambda: tts.postnet_kernel(mels[333])), 3),
                                           hip_second_ms=round(wall_ms(lambda: tts.postnet_kernel(mels[333])), 3),
                                           torch_first_ms=round(wall_ms(lambda: post_torch(mels[333])), 3),
                                           torch_second_ms=round(wall_ms(lambda: post_torch(mels[333])), 3))
        res['first_call_at_an_unseen_length'] = first
        # the outputs the two paths return, at the sizes timed
        seq_t, proj_t = tts.encode(ids)
        seq_h, proj_h, _ = tts.encode_kernel(ids)
        res['max_abs_diff'] = dict(seq=float((seq_t - seq_h).abs().max()), seq_proj=float((proj_t - proj_h).abs().max()),
                                   linear_800=float((post_torch(mels[800])[0] - tts.postnet_kernel(mels[800])[0]).abs().max()))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
