#!/usr/bin/env python
"""A/B of the TEACHER-FORCED Tacotron decoder on one MI355X (`wrnn_taco_decode_forced`: the PreNet pre-pass and the FORCED form of
wrnn_taco_batch_kernel, csrc/wrnn_taco_batch.hip) against the unchanged free-running `wrnn_taco_decode_batch` of the same S sentences.  The
protocol of scripts/gpu_taco_batch_ab.py: one process, warm, HIP events around the calls, the two paths alternating; five repeats each, minimum
and median.  S = 1, 2, 4, 8 sentences of 60-90 ids, 200 decoder steps (the free-running stop test off; the forced mel is a seeded random mel of
200 r frames).  Both paths reuse their buffers and workspaces: only the launches are timed.  The forced call's split into its two kernels comes
from one `torch.profiler` pass over five more calls (kernel durations; the events time the call as a whole: memset, pre-pass, loop).

Second part: utterances per second of `forward_gta_batch` (64 sentences of 40-103 ids, 60-149 frames) against the eager `forward_gta(kernel=False)`
loop on the same GPU (run once: it takes seconds).

    python scripts/gpu_gta_ab.py --out profiles/gta_ab.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = 'Scientists at the CERN laboratory say they have discovered a new particle. Its mass surprised everyone.'
LENGTHS = (74, 61, 88, 67, 90, 60, 81, 70)               # ids per sentence (prefixes of BASE), as scripts/gpu_taco_batch_ab.py


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_split(fn, calls):
    """mean device time (us) per call of the forced call's two kernels, from torch.profiler; None where the profiler reports no such kernel"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        tot = {'prenet': 0.0, 'loop': 0.0}
        cnt = {'prenet': 0, 'loop': 0}
        for ev in prof.events():
            name = ev.name
            dur = getattr(ev, 'device_time', None) or getattr(ev, 'cuda_time', 0.0)
            key = 'prenet' if 'wrnn_taco_prenet_kernel' in name else 'loop' if 'wrnn_taco_batch_kernel' in name else None
            if key and dur:
                tot[key] += dur
                cnt[key] += 1
        if cnt['prenet'] == 0 or cnt['loop'] == 0:
            return None
        return {k: tot[k] / cnt[k] for k in tot}
    except Exception as e:                                 # the measurement above does not depend on it
        print('torch.profiler pass failed:', e)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--utterances', type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_mel, random_tacotron_state_dict
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
    steps, r, thr = a.steps, tts.r, -1e9                  # no frame is below the threshold: the free-running sentences run all `steps`
    stream = torch.cuda.current_stream(dev).cuda_stream
    mels = [torch.zeros(steps, 80, r, device=dev) for _ in encs]
    scores = [torch.zeros(steps, e[0].size(0), device=dev) for e in encs]
    force = [torch.from_numpy(random_mel(700 + s, steps * r) * 8 - 4).to(dev).contiguous() for s in range(len(encs))]
    done = torch.zeros(8, dtype=torch.int32, device=dev)
    frames8 = (ctypes.c_int32 * 8)(*([steps * r] * 8))
    ws_b = torch.empty(int(L.wrnn_taco_batch_workspace_bytes(8)), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(int(L.wrnn_taco_forced_workspace_bytes(8, frames8, r)), dtype=torch.uint8, device=dev)

    def tables(c, S, extra=()):
        c.n = (ctypes.c_int32 * S)(*[e[0].size(0) for e in encs[:S]])
        for name, ts in (('seq', [e[0] for e in encs]), ('seq_proj', [e[1] for e in encs]), ('mel_out', mels), ('scores_out', scores)) + tuple(extra):
            setattr(c, name, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts[:S]]))

    def batch_call(S):
        c = _lib.TacoBatchCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
        c.n_sent, c.r, c.max_r, c.stop_threshold = S, r, tts.max_r, thr
        c.max_steps = (ctypes.c_int32 * S)(*([steps] * S))
        tables(c, S)
        c.steps_done, c.workspace, c.workspace_bytes, c.stream = done.data_ptr(), ws_b.data_ptr(), ws_b.numel(), stream
        return c

    def forced_call(S):
        c = _lib.TacoForcedCall()
        c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
        c.n_sent, c.r, c.max_r = S, r, tts.max_r
        c.frames = (ctypes.c_int32 * S)(*([steps * r] * S))
        tables(c, S, (('force_mel', force),))
        c.workspace, c.workspace_bytes, c.stream = ws_f.data_ptr(), ws_f.numel(), stream
        return c

    def check(rc):
        if rc != _lib.WRNN_OK:
            raise SystemExit(f'decode failed (rc={rc}): {L.wrnn_taco_last_error().decode()}')

    def clean(ws):
        st4 = (ctypes.c_uint32 * 4)()
        check(L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), stream))
        if list(st4) != [0, 0, 0, 0]:
            raise SystemExit(f'decoder kernel reported {list(st4)}')

    res = dict(device=torch.cuda.get_device_name(0), steps=steps, r=r, lengths=list(LENGTHS), reps=a.reps,
               timing='HIP events around the calls (launches only, buffers reused), free-running / forced alternating, warm; ms.  '
                      'kernels_us: mean device time of the forced call\'s two kernels over five more calls (torch.profiler)',
               free='one wrnn_taco_decode_batch (stop test off)', forced='one wrnn_taco_decode_forced (memset, PreNet pre-pass, loop)',
               model='two of ten exchange hops off the chain: about 4 us per step less (DESIGN.md section 6); a model, not a measurement')
    for S in (1, 2, 4, 8):
        bc, fc = batch_call(S), forced_call(S)
        free = lambda: check(L.wrnn_taco_decode_batch(0, ctypes.byref(w), ctypes.byref(bc)))
        forced = lambda: check(L.wrnn_taco_decode_forced(0, ctypes.byref(w), ctypes.byref(fc)))
        for _ in range(2):
            free()
            clean(ws_b)
            forced()
            clean(ws_f)
        assert [int(k) for k in done.cpu()[:S]] == [steps] * S
        tf, tg = [], []
        for _ in range(a.reps):
            tf.append(event_ms(free))
            tg.append(event_ms(forced))
        clean(ws_b)
        clean(ws_f)
        split = kernel_split(forced, 5)
        clean(ws_f)
        f = lambda v: dict(min_ms=round(min(v), 4), median_ms=round(statistics.median(v), 4), max_ms=round(max(v), 4),
                           us_per_step_min=round(min(v) * 1e3 / steps, 2), us_per_step_median=round(statistics.median(v) * 1e3 / steps, 2))
        row = dict(free=f(tf), forced=f(tg), saved_us_per_step_min=round((min(tf) - min(tg)) * 1e3 / steps, 2),
                   saved_us_per_step_median=round((statistics.median(tf) - statistics.median(tg)) * 1e3 / steps, 2),
                   # the forced call beats the free-running one by more than the spread of the repeats: its slowest repeat under their fastest
                   forced_wins_beyond_spread=bool(max(tg) < min(tf)))
        if split is not None:
            row['kernels_us'] = dict(prenet_prepass=round(split['prenet'], 1), loop=round(split['loop'], 1),
                                     loop_us_per_step=round(split['loop'] / steps, 2), prepass_us_per_step=round(split['prenet'] / steps, 3))
        res[f'S={S}'] = row

    # ---- utterances per second: forward_gta_batch against the eager loop ----
    U = a.utterances
    sents = [ids[:40 + u % 64] for u in range(U)]
    gmels = [random_mel(900 + u, 60 + (37 * u) % 90) * 8 - 4 for u in range(U)]
    total_frames = sum(m.shape[1] for m in gmels)
    corpus = dict(utterances=U, ids='40..103', frames='60..149', total_frames=total_frames)
    for name, kw in (('kernel_cbhg_kernel', dict(cbhg_kernel=True)), ('kernel_torch_front', dict(cbhg_kernel=False))):
        tts.forward_gta_batch(sents, gmels, **kw)
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = tts.forward_gta_batch(sents, gmels, **kw)
            ts.append(time.perf_counter() - t0)
        corpus[name] = dict(min_s=round(min(ts), 4), median_s=round(statistics.median(ts), 4), utt_per_s_min_time=round(U / min(ts), 1),
                            utt_per_s_median=round(U / statistics.median(ts), 1))
    tts.forward_gta(sents[0], gmels[0], kernel=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eager = [tts.forward_gta(s, m, kernel=False) for s, m in zip(sents, gmels)]
    te = time.perf_counter() - t0
    corpus['eager'] = dict(seconds=round(te, 3), utt_per_s=round(U / te, 2), runs=1, us_per_step=round(te * 1e6 / (total_frames / r), 1))
    corpus['speedup_cbhg_kernel_median'] = round(te / corpus['kernel_cbhg_kernel']['median_s'], 1)
    corpus['max_abs_kernel_minus_eager_gta'] = float(max(np.abs(o[0] - e[0]).max() for o, e in zip(outs, eager)))
    res['corpus'] = corpus
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
