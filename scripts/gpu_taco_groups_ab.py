#!/usr/bin/env python
"""A/B of two sentence groups per launch of the batched Tacotron decoder on one MI355X: ONE `wrnn_taco_decode_batch_groups` /
`wrnn_taco_decode_forced_groups` call of 2 x S sentences (csrc/wrnn_taco_batch.hip, the GROUPED instantiations: 256 workgroups) against TWO
back-to-back plain calls of S sentences each -- what the library does with 2 S sentences without the grouped entry points: the baseline.  The
protocol is that of scripts/gpu_taco_batch_ab.py: one process, warm, HIP events around the calls, the contenders alternating, five repeats each,
minimum and median; S = 1, 2, 4, 8 sentences of 60-90 ids per group, 200 decoder steps (free-running: the stop test off; forced: 200 frames).
Both forms.  Every contender has its own output buffers and workspaces and reuses them: only the launches are timed.

The placement of the groups on the device is a compile-time switch of the library (WRNN_TACO_GROUP_PLACEMENT, csrc/wrnn_taco_batch.hip).  To
time both in one session, build a second copy of the library with the other value and pass it as --alt_so:

    WRNN_SO_OUT=/tmp/libwavernn_amd_alt.so wavernn_amd/csrc/build.sh -DWRNN_TACO_GROUP_PLACEMENT=1
    python scripts/gpu_taco_groups_ab.py --alt_so /tmp/libwavernn_amd_alt.so --out profiles/taco_groups_ab.json

Last part: the 64-utterance `forward_gta_batch` set of scripts/gpu_gta_ab.py (40-103 ids, 60-149 frames) with groups=1 and groups=2, alternating.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE = 'Scientists at the CERN laboratory say they have discovered a new particle. Its mass surprised everyone.'
LENGTHS = (74, 61, 88, 67, 90, 60, 81, 70)               # ids per sentence (prefixes of BASE): 60-90, as the reference's sentences.txt
PLACEMENTS = {0: 'contiguous', 1: 'interleaved'}


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
    ap.add_argument('--alt_so', default=None, help='a copy of the library built with the other WRNN_TACO_GROUP_PLACEMENT')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--utterances', type=int, default=64)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    from wavernn_amd import _lib
    from wavernn_amd.synthetic import random_mel, random_tacotron_state_dict
    from wavernn_amd.tacotron import TacotronInference, text_to_ids
    L = _lib.lib()
    libs = [L]
    if a.alt_so:
        alt = ctypes.CDLL(os.path.abspath(a.alt_so))
        alt.wrnn_taco_last_error.restype = ctypes.c_char_p
        for name in ('wrnn_taco_decode_batch_groups', 'wrnn_taco_decode_forced_groups', 'wrnn_debug_taco_group_of'):
            getattr(alt, name).argtypes = getattr(L, name).argtypes
        libs.append(alt)

    def placement(lib):
        g, l = ctypes.c_int32(), ctypes.c_int32()
        return PLACEMENTS[lib.wrnn_debug_taco_group_of(0, ctypes.byref(g), ctypes.byref(l))]
    names = [placement(lib) for lib in libs]
    assert len(set(names)) == len(names), f'--alt_so has the placement of the shipped library ({names[0]})'

    dev = torch.device('cuda', 0)
    shapes = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'tacotron_shapes.json')))
    tts = TacotronInference(random_tacotron_state_dict(3, shapes), device=dev)
    w = tts.decoder_weights()
    ids = text_to_ids(BASE)
    assert len(ids) >= max(LENGTHS)
    with torch.no_grad():
        enc8 = [tuple(t[0].contiguous() for t in tts.encode(ids[:n])) for n in LENGTHS]
    steps, r, thr = a.steps, tts.r, -1e9                  # no frame is below the threshold: the free-running sentences run all `steps`
    stream = torch.cuda.current_stream(dev).cuda_stream
    force8 = [torch.from_numpy(random_mel(700 + s, steps * r) * 8 - 4).to(dev).contiguous() for s in range(8)]
    frames8 = (ctypes.c_int32 * 8)(*([steps * r] * 8))
    keep = []

    def group(forced, S, shift):
        """A call struct of S sentences (group B: the same eight sentences rotated by `shift`) with outputs and a workspace of its own."""
        order = [(s + shift) % 8 for s in range(S)]
        encs = [enc8[s] for s in order]
        mels = [torch.zeros(steps, 80, r, device=dev) for _ in encs]
        scores = [torch.zeros(steps, e[0].size(0), device=dev) for e in encs]
        tabs = [('seq', [e[0] for e in encs]), ('seq_proj', [e[1] for e in encs]), ('mel_out', mels), ('scores_out', scores)]
        if forced:
            c = _lib.TacoForcedCall()
            c.struct_bytes = ctypes.sizeof(_lib.TacoForcedCall)
            c.frames = (ctypes.c_int32 * S)(*([steps * r] * S))
            tabs.append(('force_mel', [force8[s] for s in order]))
            ws = torch.empty(int(L.wrnn_taco_forced_workspace_bytes(8, frames8, r)), dtype=torch.uint8, device=dev)
            done = None
        else:
            c = _lib.TacoBatchCall()
            c.struct_bytes = ctypes.sizeof(_lib.TacoBatchCall)
            c.stop_threshold = thr
            c.max_steps = (ctypes.c_int32 * S)(*([steps] * S))
            ws = torch.empty(int(L.wrnn_taco_batch_workspace_bytes(8)), dtype=torch.uint8, device=dev)
            done = torch.zeros(8, dtype=torch.int32, device=dev)
            c.steps_done = done.data_ptr()
        c.n_sent, c.r, c.max_r = S, r, tts.max_r
        c.n = (ctypes.c_int32 * S)(*[e[0].size(0) for e in encs])
        for name, ts in tabs:
            setattr(c, name, (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts]))
        c.workspace, c.workspace_bytes, c.stream = ws.data_ptr(), ws.numel(), stream
        keep.append((mels, scores, ws, done))
        return c, ws, mels, done

    def check(rc, lib=L):
        if rc != _lib.WRNN_OK:
            raise SystemExit(f'decode failed (rc={rc}): {lib.wrnn_taco_last_error().decode()}')

    def clean(ws):
        st4 = (ctypes.c_uint32 * 4)()
        check(L.wrnn_taco_status(ws.data_ptr(), ctypes.byref(st4), stream))
        if list(st4) != [0, 0, 0, 0]:
            raise SystemExit(f'decoder kernel reported {list(st4)}')

    res = dict(device=torch.cuda.get_device_name(0), steps=steps, r=r, lengths=list(LENGTHS), reps=a.reps, shipped_placement=names[0],
               timing='HIP events around the calls (launches only, buffers reused), the contenders alternating, warm; ms',
               serial='two back-to-back plain calls of S sentences each (wrnn_taco_decode_batch / wrnn_taco_decode_forced)',
               grouped='one wrnn_taco_decode_batch_groups / wrnn_taco_decode_forced_groups call of 2 x S sentences',
               model='the groups share no data: a grouped call costs at least one plain call of S and at most two (ratio 1..2); not a measurement')
    f = lambda v: dict(min_ms=round(min(v), 4), median_ms=round(statistics.median(v), 4), max_ms=round(max(v), 4),
                       us_per_step_min=round(min(v) * 1e3 / steps, 2), us_per_step_median=round(statistics.median(v) * 1e3 / steps, 2))
    for forced in (False, True):
        form = 'forced' if forced else 'free'
        plain = L.wrnn_taco_decode_forced if forced else L.wrnn_taco_decode_batch
        struct = _lib.TacoForcedCall if forced else _lib.TacoBatchCall
        for S in (1, 2, 4, 8):
            sa, sb = group(forced, S, 0), group(forced, S, 3)                      # the serial contender's two calls
            contenders = {'serial': (lambda sa=sa, sb=sb: [check(plain(0, ctypes.byref(w), ctypes.byref(c[0]))) for c in (sa, sb)], [sa, sb])}
            for lib, name in zip(libs, names):
                ga, gb = group(forced, S, 0), group(forced, S, 3)
                table = (ctypes.POINTER(struct) * 2)(ctypes.pointer(ga[0]), ctypes.pointer(gb[0]))
                entry = lib.wrnn_taco_decode_forced_groups if forced else lib.wrnn_taco_decode_batch_groups
                contenders[f'grouped_{name}'] = (lambda entry=entry, table=table, lib=lib: check(entry(0, ctypes.byref(w), table, 2), lib), [ga, gb])
            for _ in range(2):
                for fn, groups in contenders.values():
                    fn()
                    for g in groups:
                        clean(g[1])
            # every contender computed the same thing
            ref = contenders['serial'][1]
            for name, (_, groups) in contenders.items():
                for g, g0 in zip(groups, ref):
                    assert all(torch.equal(x, y) for x, y in zip(g[2], g0[2])), (form, S, name)
                    assert forced or [int(k) for k in g[3].cpu()[:S]] == [steps] * S
            times = {name: [] for name in contenders}
            for _ in range(a.reps):
                for name, (fn, _) in contenders.items():
                    times[name].append(event_ms(fn))
            for _, groups in contenders.values():
                for g in groups:
                    clean(g[1])
            row = {name: f(v) for name, v in times.items()}
            for name in names:
                v = times[f'grouped_{name}']
                row[f'ratio_min_{name}'] = round(min(times['serial']) / min(v), 3)
                row[f'ratio_median_{name}'] = round(statistics.median(times['serial']) / statistics.median(v), 3)
                # the grouped call beats the two serial calls by more than the spread of the repeats: its slowest repeat under their fastest
                row[f'grouped_{name}_wins_beyond_spread'] = bool(max(v) < min(times['serial']))
            res[f'{form} S={S}'] = row
            print(form, S, json.dumps(row), flush=True)
            del contenders
            keep.clear()

    # ---- the 64-utterance forward_gta_batch set of scripts/gpu_gta_ab.py, groups = 1 against groups = 2 (the shipped placement) ----
    U = a.utterances
    sents = [ids[:40 + u % 64] for u in range(U)]
    gmels = [random_mel(900 + u, 60 + (37 * u) % 90) * 8 - 4 for u in range(U)]
    corpus = dict(utterances=U, ids='40..103', frames='60..149', total_frames=sum(m.shape[1] for m in gmels), cbhg_kernel=True, max_batch=8)
    ts = {1: [], 2: []}
    outs = {}
    for G in (1, 2):
        outs[G] = tts.forward_gta_batch(sents, gmels, cbhg_kernel=True, groups=G)
        corpus[f'groups={G}_launches'] = [list(x) for x in tts.last_decode_groups]
    assert all((x == y).all() for o, p in zip(outs[1], outs[2]) for x, y in zip(o, p)), 'groups=2 changed a result'
    for _ in range(a.reps):
        for G in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tts.forward_gta_batch(sents, gmels, cbhg_kernel=True, groups=G)
            ts[G].append(time.perf_counter() - t0)
    for G in (1, 2):
        corpus[f'groups={G}'] = dict(min_s=round(min(ts[G]), 4), median_s=round(statistics.median(ts[G]), 4), max_s=round(max(ts[G]), 4),
                                     utt_per_s_min_time=round(U / min(ts[G]), 1), utt_per_s_median=round(U / statistics.median(ts[G]), 1))
    corpus['ratio_median'] = round(statistics.median(ts[1]) / statistics.median(ts[2]), 3)
    corpus['groups=2_wins_beyond_spread'] = bool(max(ts[2]) < min(ts[1]))
    res['corpus'] = corpus
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(line + '\n')


if __name__ == '__main__':
    main()
