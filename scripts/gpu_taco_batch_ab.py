#!/usr/bin/env python
"""A/B of the Tacotron decoder loop for a list of sentences on one MI355X: ONE `wrnn_taco_decode_batch` call for S sentences
(csrc/wrnn_taco_batch.hip) against S back-to-back `wrnn_taco_decode(variant=2)` calls (the single-sentence register-resident kernel: the
yardstick).  One process, warm, HIP events around the calls, the two paths alternating; five repeats each, minimum and median.  S = 1, 2, 4,
8 sentences of 60-90 ids, 200 decoder steps, the stop test off (threshold below every frame).  Random-init weights of the reference's
architecture (tests/golden/tacotron_shapes.json).  Both paths reuse their buffers and workspaces: only the launches are timed.

    python scripts/gpu_taco_batch_ab.py --out profiles/taco_batch_ab.json
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
    ap.add_argument('--steps', type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    L = _lib.lib()
    dev = torch.device('cuda', 0)
    shapes = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device=dev)
    w = tts.decoder_weights()
    ids = text_to_ids(BASE)
    assert len(ids) >= max(LENGTHS)
    with torch.no_grad():
        encs = [tuple(t[0].contiguous() for t in tts.encode(ids[:n])) for n in LENGTHS]
    steps, thr = a.steps, -1e9                            # no frame is below it: every sentence runs all `steps`
    stream = torch.cuda.current_stream(dev).cuda_stream
    mels = [torch.zeros(steps, 80, tts.r, device=dev) for _ in encs]
    scores = [torch.zeros(steps, e[0].size(0), device=dev) for e in encs]
    done = torch.zeros(8, dtype=torch.int32, device=dev)
    ws1 = torch.empty(int(L.wrnn_taco_workspace_bytes()), dtype=torch.uint8, device=dev)
    ws8 = torch.empty(int(L.wrnn_taco_batch_workspace_bytes(8)), dtype=torch.uint8, device=dev)

    singles = []
    for s, (seq, proj) in enumerate(encs):
        c = _lib.TacoCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoCall)
        c.n, c.r, c.max_r, c.max_steps, c.stop_threshold, c.variant = seq.size(0), tts.r, tts.max_r, steps, thr, 2
        c.seq, c.seq_proj, c.mel_out, c.scores_out = seq.data_ptr(), proj.data_ptr(), mels[s].data_ptr(), scores[s].data_ptr()
        c.steps_done, c.workspace, c.workspace_bytes, c.stream = done.data_ptr() + 4 * s, ws1.data_ptr(), ws1.numel(), stream
        singles.append(c)

    def batch_call(S):
        c = _lib.TacoBatchCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
        c.n_sent, c.r, c.max_r, c.stop_threshold = S, tts.r, tts.max_r, thr
        c.n = (ctypes.c_int32 * S)(*[e[0].size(0) for e in encs[:S]])
        c.max_steps = (ctypes.c_int32 * S)(*([steps] * S))
        for name, ts in (('seq', [e[0] for e in encs]), ('seq_proj', [e[1] for e in encs]), ('mel_out', mels), ('scores_out', scores)):
            setattr(c, name, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts[:S]]))
        c.steps_done, c.workspace, c.workspace_bytes, c.stream = done.data_ptr(), ws8.data_ptr(), ws8.numel(), stream
        return c

    def check(rc):
        if rc != _lib.WRNN_OK:
            raise SystemExit(f'decode failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')

    def clean(ws):
        st4 = (ctypes.c_uint32 * 4)()
        check(L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), stream))
        if list(st4) != [0, 0, 0, 0]:
            raise SystemExit(f'decoder kernel reported {list(st4)}')

    res = dict(device=torch.cuda.get_device_name(0), steps=steps, lengths=list(LENGTHS), reps=a.reps,
               timing='HIP events around the calls (launches only, buffers reused), serial / batched alternating, warm; ms',
               serial='S back-to-back wrnn_taco_decode(variant=2)', batched='one wrnn_taco_decode_batch', model_us_per_step='<= 20 + 8 S (DESIGN.md section 6)')
    for S in (1, 2, 4, 8):
        bc = batch_call(S)
        serial = lambda: [check(L.wrnn_taco_decode(0, ctypes.byref(w), ctypes.byref(c))) for c in singles[:S]]
        batched = lambda: check(L.wrnn_taco_decode_batch(0, ctypes.byref(w), ctypes.byref(bc)))
        for _ in range(2):
            serial()
            clean(ws1)
            batched()
            clean(ws8)
        assert [int(k) for k in done.cpu()[:S]] == [steps] * S
        ts, tb = [], []
        for _ in range(a.reps):
            ts.append(event_ms(serial))
            tb.append(event_ms(batched))
        clean(ws1)
        clean(ws8)
        f = lambda v: dict(min_ms=round(min(v), 4), median_ms=round(statistics.median(v), 4), max_ms=round(max(v), 4),
                           us_per_step_min=round(min(v) * 1e3 / steps, 2), us_per_step_median=round(statistics.median(v) * 1e3 / steps, 2))
        res[f'S={S}'] = dict(serial=f(ts), batched=f(tb), ratio_min=round(min(ts) / min(tb), 3), ratio_median=round(statistics.median(ts) / statistics.median(tb), 3),
                             # the batched call beats the serial calls by more than the spread of the repeats: its slowest repeat under their fastest
                             batched_wins_beyond_spread=bool(max(tb) < min(ts)))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
