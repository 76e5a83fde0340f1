"""Teacher-forced scoring: the negative log-likelihood a WaveRNN model gives to real audio, on the kernels that generate.

The reference asks this question in training and validation: `WaveRNN.forward(x, m)` (models/fatchord_version.py:131-167) under
`F.cross_entropy` (RAW) or `discretized_mix_logistic_loss` (MOL), train_wavernn.py:83, :123.  Here the forward is a loop call with
`wrnn_options.force_x` (the waveform is fed back instead of the samples drawn) and `wrnn_options.logits` (fc3's output of every step), on whatever
loop kernel the model's `loop_algo` plans -- the block-sparse one for a pruned pack --, followed by one `wrnn_nll` launch on the same stream.

  prepare_targets   a waveform -> the values the loop is fed and scored against (host numpy: preprocess.py:43-45, utils/dsp.py:8-15, :92-96)
  chunk_by_bytes    utterances -> chunks whose logits stay under a byte budget, sorted by length
  segment_table     the segment table of a chunk's ragged utterances, one UNFOLDED segment each
  score_corpus      n utterances -> one loop call + one loss launch per chunk
  score             one utterance (`WaveRNN.score`)

No gradients; no folding (a fold restarts the state and scores its overlaps twice, which is not the reference's forward).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

LN2 = math.log(2.0)


def float_2_label(x, bits):
    """utils/dsp.py:12-15 and the `.astype(np.int64)` of preprocess.py:47: [-1, 1] -> integer labels 0 .. 2**bits - 1 (truncated)."""
    x = np.asarray(x)
    if x.size and np.abs(x).max() > 1.0:
        raise ValueError('the waveform must lie in [-1, 1]')
    return ((x + 1.) * (2 ** bits - 1) / 2).clip(0, 2 ** bits - 1).astype(np.int64)


def encode_mu_law(x, mu):
    """utils/dsp.py:92-96 (+ preprocess.py:47): [-1, 1] -> mu-law labels 0 .. mu - 1."""
    x = np.asarray(x)
    if x.size and np.abs(x).max() > 1.0:
        raise ValueError('the waveform must lie in [-1, 1]')
    mu = mu - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    return np.floor((fx + 1) / 2 * mu + 0.5).astype(np.int64)


def labels_to_values(labels, bits):
    """`label_2_float(labels.float(), bits)` as utils/dataset.py:88-91 forms it (float32 arithmetic): 2 idx / (2**bits - 1) - 1."""
    return np.float32(2) * np.asarray(labels).astype(np.float32) / np.float32(2 ** bits - 1) - np.float32(1)


def prepare_targets(wav, mode, bits=9, mu_law=True):
    """(labels int64, values float32) of a waveform: the values are both what the loop is fed (`force_x`) and what `wrnn_nll` scores (`target`).
    MOL: the 16-bit grid; RAW: 2**bits classes, mu-law encoded when `mu_law`.  An integer array is taken as labels already."""
    wav = np.asarray(wav)
    if wav.ndim != 1:
        raise ValueError('a waveform is a 1-D array')
    bits = 16 if mode == 'MOL' else int(bits)
    if np.issubdtype(wav.dtype, np.integer):
        labels = wav.astype(np.int64)
        if labels.size and (labels.min() < 0 or labels.max() > 2 ** bits - 1):
            raise ValueError(f'labels outside 0..{2 ** bits - 1}')
    elif mode == 'RAW' and mu_law:
        labels = encode_mu_law(wav, 2 ** bits)
    else:
        labels = float_2_label(wav, bits)
    return labels, labels_to_values(labels, bits)


def chunk_by_bytes(steps, n_classes, budget):
    """Cut utterances of `steps[u]` counted steps into chunks whose logits -- T * n * n_classes * 4 bytes, T the chunk's longest -- stay under
    `budget`.  The utterances are sorted by length first (T stays tight); returns a list of index lists (the caller's indices), none empty, every
    utterance in exactly one.  One utterance that does not fit alone: ValueError naming the bytes it needs."""
    steps = [int(s) for s in steps]
    order = sorted(range(len(steps)), key=lambda u: (steps[u], u))
    chunks, cur = [], []
    for u in order:                       # ascending: the utterance being added is the chunk's longest
        need = steps[u] * int(n_classes) * 4
        if need > budget:
            raise ValueError(f'utterance {u}: {steps[u]} steps x {n_classes} classes need {need} bytes of logits, over the budget of {budget} '
                             '(model.score_logits_bytes)')
        if cur and need * (len(cur) + 1) > budget:
            chunks.append(cur)
            cur = []
        cur.append(u)
    if cur:
        chunks.append(cur)
    return chunks


def segment_table(frames, steps, hop):
    """(seg_pos, seg_lim) int32 of a chunk whose utterances' conditioning (frames[u] * hop positions each) is concatenated: seg_pos = o_u,
    seg_lim = o_u + steps[u]."""
    frames, steps = np.asarray(frames, np.int64), np.asarray(steps, np.int64)
    if np.any(steps < 1) or np.any(steps > frames * hop):
        raise ValueError('an utterance counts 1 .. frames * hop steps')
    off = np.concatenate([[0], np.cumsum(frames * hop)[:-1]])
    if int(off[-1]) + int(frames[-1]) * hop + int(steps.max()) >= 2 ** 31:
        raise ValueError('concatenated conditioning exceeds int32 positions; lower model.score_logits_bytes')
    return off.astype(np.int32), (off + steps).astype(np.int32)


def result(nll_sum, steps, per_step=None):
    mean = float(nll_sum) / int(steps)
    r = dict(nll_sum=float(nll_sum), steps=int(steps), nll_mean=mean, bits_per_sample=mean / LN2)
    if per_step is not None:
        r['per_step'] = per_step
    return r


def nll_on_device(lib, dev_index, mode, logits, target, seg_len, per_step):
    """One `wrnn_nll` launch on the current stream: logits (T, n, C), target (n, T) float32 CUDA, seg_len (n,) int32 CUDA -> (nll or None, sum)."""
    T, n, C = logits.shape
    nll = torch.empty(n, T, dtype=torch.float32, device=logits.device) if per_step else None
    total = torch.empty(n, dtype=torch.float64, device=logits.device)
    c = _lib.NllCall(mode=_lib.MODE_MOL if mode == 'MOL' else _lib.MODE_RAW, n_classes=C, n_segments=n, T=T, logits=logits.data_ptr(),
                     target=target.data_ptr(), seg_len=seg_len.data_ptr(), nll=None if nll is None else nll.data_ptr(), sum=total.data_ptr(),
                     stream=torch.cuda.current_stream(logits.device).cuda_stream)
    _lib.check(lib.wrnn_nll(dev_index, ctypes.byref(c)), 'wrnn_nll')
    return nll, total


def score_corpus(model, mels, wavs, mu_law=None, per_step=False, algo=None, timings=None):
    """Score n utterances under `model` (a `wavernn_amd.WaveRNN` on a HIP device): mels[u] (1, feat, N_u) or (feat, N_u), wavs[u] a float waveform in
    [-1, 1] (or integer labels) at the model's rate.  Utterance u counts min(len(wav_u), N_u * hop) steps: step t is scored against wav[t] and fed
    wav[t - 1] (0 in front), from a zero state, over the mel padded as `generate` pads it -- the reference's `forward(x, m)` with x = [0, wav[:-1]].
    The utterances of a chunk (`chunk_by_bytes` under `model.score_logits_bytes`) are the segments of one loop call on `model.loop_algo` (algo:
    another one for this call); one `wrnn_nll` launch follows it.  Returns a list of dicts in the caller's order: nll_sum, steps, nll_mean (nats per
    sample), bits_per_sample [, per_step: float32 (steps,)].  timings: optional dict, receives loop_ms / loss_ms (HIP events, summed over the chunks)."""
    device = next(model.parameters()).device
    model._require_hip_device(device)
    if len(mels) != len(wavs) or not len(mels):
        raise ValueError('one waveform per mel, at least one')
    mode, hop = model.mode, model.hop_length
    mu_law = (True if mu_law is None else bool(mu_law)) if mode == 'RAW' else False
    bits = int(round(math.log2(model.n_classes))) if mode == 'RAW' else 16
    algo = model.loop_algo if algo is None else algo
    was_training = model.training
    model.eval()
    mels = [torch.as_tensor(m) for m in mels]
    mels = [m.unsqueeze(0) if m.dim() == 2 else m for m in mels]
    frames = [int(m.size(-1)) for m in mels]
    values = [prepare_targets(w, mode, bits, mu_law)[1] for w in wavs]
    steps = [min(len(v), f * hop) for v, f in zip(values, frames)]
    if min(steps) < 1:
        raise ValueError('every utterance needs at least one sample and one frame')
    budget = int(getattr(model, 'score_logits_bytes', 8 << 30))
    out = [None] * len(mels)
    eng = model._loop_engine()
    loop_ms = loss_ms = 0.0
    with torch.no_grad():
        for utts in chunk_by_bytes(steps, model.n_classes, budget):
            fr, st = [frames[u] for u in utts], [steps[u] for u in utts]
            seg_pos, seg_lim = segment_table(fr, st, hop)
            n, T = len(utts), max(st)
            # conditioning of the chunk's utterances, concatenated (each starts on a frame boundary): the pre-loop path of generate_corpus
            if getattr(model, 'pre_algo', 'torch') == 'native':
                pre = model._pre_engine()
                mels_up = torch.empty(sum(fr) * hop, mels[utts[0]].size(1), dtype=torch.float32, device=device)
                aux = torch.empty(sum(fr), 4 * model.aux_dims, dtype=torch.float32, device=device)
                jobs = [(mels[u], mels_up[int(p):int(p) + f * hop], aux[int(p) // hop:int(p) // hop + f]) for u, p, f in zip(utts, seg_pos, fr)]
                pre.upsample_many(jobs, rows=False, streams=int(getattr(model, 'pre_streams', 8)), batched=bool(getattr(model, 'pre_batched', True)))
            else:
                ups, auxs = zip(*[model.conditioning(mels[u])[:2] for u in utts])
                mels_up, aux = torch.cat(ups).contiguous(), torch.cat(auxs).contiguous()
            x = np.zeros((n, T), np.float32)
            for k, u in enumerate(utts):
                x[k, :st[k]] = values[u][:st[k]]
            x = torch.from_numpy(x).to(device)
            lens = torch.from_numpy(np.asarray(st, np.int32)).to(device)
            # noise=None: the library draws the sampling noise itself (the samples are discarded: force_x replaces them) -- no noise tensor
            _, logits = eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, None, hop, algo=algo, force_x=x, want_logits=True, check=False)
            if timings is not None:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
            nll, total = nll_on_device(eng.lib, eng._dev_index, mode, logits, x, lens, per_step)
            if timings is not None:
                ev[1].record()
            eng.status()                  # synchronises the stream; raises if a loop kernel gave up
            model.last_loop_ms, model.last_loop_kernel = eng.last_loop_ms(), eng.last_loop_kernel()
            if timings is not None:
                loop_ms += model.last_loop_ms
                loss_ms += ev[0].elapsed_time(ev[1])
            total = total.cpu().numpy()
            nll = nll.cpu().numpy() if per_step else None
            for k, u in enumerate(utts):
                out[u] = result(total[k], st[k], nll[k, :st[k]].copy() if per_step else None)
    if timings is not None:
        timings['loop_ms'], timings['loss_ms'] = loop_ms, loss_ms
    if was_training:
        model.train()
    return out


def score(model, mels, wav, mu_law=None, per_step=False):
    """`WaveRNN.score`: one utterance, unfolded (B = 1, T = the counted steps)."""
    return score_corpus(model, [mels], [wav], mu_law=mu_law, per_step=per_step)[0]
