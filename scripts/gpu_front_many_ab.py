#!/usr/bin/env python
"""A/B of Tacotron's encoder and post-net for a list of sentences on one MI355X: ONE `wrnn_taco_encode_many` / `wrnn_taco_postnet_many` call for S
sentences (csrc/wrnn_cbhg.hip) against S back-to-back `wrnn_taco_encode` / `wrnn_taco_postnet` calls (what `generate_batch(cbhg_kernel=True)` did
before: the yardstick).  One process, warm, HIP events around the calls, the two paths alternating; five repeats each, minimum and median.
S = 1, 2, 4, 8; `encode` on sentences of 60-90 ids, the post-net at 200 and at 800 frames per sentence.  Random-init weights of the reference's
architecture (tests/golden/tacotron_shapes.json).  Both paths reuse their buffers and workspaces: only the launches are timed.  The outputs of the
two paths are compared bit for bit before anything is timed.

    python scripts/gpu_front_many_ab.py --out profiles/front_many_ab.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = 'Scientists at the CERN laboratory say they have discovered a new particle. Its mass surprised everyone.'
LENGTHS = (74, 61, 88, 67, 90, 60, 81, 70)               # ids per sentence (prefixes of BASE): 60-90, as the reference's sentences.txt


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    L = _lib.lib()
    dev = torch.device('cuda', 0)
    shapes = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device=dev)
    h = tts._front_handle()
    assert h is not None
    stream = torch.cuda.current_stream(dev).cuda_stream
    ids = text_to_ids(BASE)
    assert len(ids) >= max(LENGTHS)

    def check(rc, what):
        if rc != _lib.WRNN_OK:
            raise SystemExit(f'{what} failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')

    def workspace(lengths):
        n = (ctypes.c_int32 * len(lengths))(*lengths)
        many = int(L.wrnn_taco_front_workspace_bytes_many(h, n, len(lengths)))
        one = max(int(L.wrnn_taco_front_workspace_bytes(h, k)) for k in lengths)
        return n, torch.empty(many, dtype=torch.uint8, device=dev), torch.empty(one, dtype=torch.uint8, device=dev)

    def encode_paths(S):
        lengths = list(LENGTHS[:S])
        rows, offs = sum(lengths), [sum(lengths[:s]) for s in range(S)]
        n, ws_many, ws_one = workspace(lengths)
        ids_d = torch.tensor([i for k in lengths for i in ids[:k]], dtype=torch.int32).to(dev)
        out = {p: (torch.zeros(rows, 256, device=dev), torch.zeros(rows, 256, device=dev)) for p in ('serial', 'many')}

        def serial():
            seq, proj = out['serial']
            for s, k in enumerate(lengths):
                check(L.wrnn_taco_encode(h, ids_d.data_ptr() + 4 * offs[s], k, seq.data_ptr() + 1024 * offs[s], proj.data_ptr() + 1024 * offs[s], None,
                                         ws_one.data_ptr(), ws_one.numel(), stream), 'wrnn_taco_encode')

        def many():
            seq, proj = out['many']
            check(L.wrnn_taco_encode_many(h, ids_d.data_ptr(), n, S, seq.data_ptr(), proj.data_ptr(), None, ws_many.data_ptr(), ws_many.numel(), stream),
                  'wrnn_taco_encode_many')
        return serial, many, out

    def postnet_paths(S, N):
        lengths = [N] * S
        n, ws_many, ws_one = workspace(lengths)
        g = torch.Generator().manual_seed(7)
        mels = [torch.randn(80, N, generator=g).to(dev) for _ in range(S)]
        ptrs = (ctypes.c_void_p * S)(*[m.data_ptr() for m in mels])
        out = {p: (torch.zeros(S * N, 80, device=dev),) for p in ('serial', 'many')}

        def serial():
            lin, = out['serial']
            for s, m in enumerate(mels):
                check(L.wrnn_taco_postnet(h, m.data_ptr(), N, lin.data_ptr() + 320 * N * s, None, ws_one.data_ptr(), ws_one.numel(), stream), 'wrnn_taco_postnet')

        def many():
            lin, = out['many']
            check(L.wrnn_taco_postnet_many(h, ptrs, n, S, lin.data_ptr(), None, ws_many.data_ptr(), ws_many.numel(), stream), 'wrnn_taco_postnet_many')
        return serial, many, out, mels

    res = dict(device=torch.cuda.get_device_name(0), lengths=list(LENGTHS), reps=a.reps,
               timing='HIP events around the calls (launches only, buffers reused), serial / many alternating, warm; ms',
               serial='S back-to-back wrnn_taco_encode / wrnn_taco_postnet', many='one wrnn_taco_encode_many / wrnn_taco_postnet_many')
    stages = [('encode_60_90_ids', lambda S: encode_paths(S)), ('postnet_200_frames', lambda S: postnet_paths(S, 200)),
              ('postnet_800_frames', lambda S: postnet_paths(S, 800))]
    for name, make in stages:
        res[name] = {}
        for S in (1, 2, 4, 8):
            made = make(S)
            serial, many, out = made[:3]
            for _ in range(2):
                serial()
                many()
            torch.cuda.synchronize()
            same = all(torch.equal(x, y) for x, y in zip(out['serial'], out['many']))
            if not same:
                raise SystemExit(f'{name} S={S}: the _many call and the serial calls differ')
            ts, tm = [], []
            for _ in range(a.reps):
                ts.append(event_ms(serial))
                tm.append(event_ms(many))
            f = lambda v: dict(min_ms=round(min(v), 4), median_ms=round(statistics.median(v), 4), max_ms=round(max(v), 4))
            res[name][f'S={S}'] = dict(serial=f(ts), many=f(tm), bitwise_equal=same, ratio_min=round(min(ts) / min(tm), 3),
                                       ratio_median=round(statistics.median(ts) / statistics.median(tm), 3),
                                       # the one call beats the serial calls by more than the spread of the repeats: its slowest repeat under their fastest
                                       many_wins_beyond_spread=bool(max(tm) < min(ts)))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
