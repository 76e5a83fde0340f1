"""`python -m wavernn_amd.gta_tacotron --tts_weights W.pyt --path DATA` -- ground-truth-aligned (GTA) mels for vocoder training and scoring: what
the reference's `train_tacotron.py --force_gta` (:178-199) writes to DATA/gta, produced by the teacher-forced decoder kernel
(`TacotronInference.forward_gta_batch`, `wrnn_taco_decode_forced`, csrc/wrnn_taco_batch.hip) instead of the reference's per-frame Python loop.

Reads the reference's dataset layout: DATA/dataset.pkl (a list of (id, mel_len)), DATA/text_dict.pkl (id -> text) and DATA/mel/<id>.npy ((80, N),
values in [0, 1]).  Every utterance of dataset.pkl is processed (the reference's loader drops those longer than `tts_max_mel_len`).  The decoder is
fed `mel * 8 - 4`; written is `(gta[:, :N] + 4) / 8` as float32 to <out>/<id>.npy (default DATA/gta), where `gta` is what the reference's script
calls so: the SECOND return of the forward (`_, gta, _ = model(x, mels)`, :187 -- the post-net output, 80 bins because fft_bins = num_mels), the
same return `gen_tacotron.py:142` hands the vocoder.  This is train_tacotron.py:191-194 exactly.

Text goes through `text_to_ids`: the same limited cleaning as `gen_tacotron` here (lowercase, whitespace; no number or abbreviation expansion).

Two deliberate differences from the reference's script (see `TacotronInference.forward_gta`).  MODE: `create_gta_features` calls `model(x, mels)`
without `generate_gta`, so the checked-in script runs in train mode -- PreNet dropout, batch statistics in the batch norms; this is the eval form
the signature offers, the only deterministic one.  PADDING: the reference pads a batch's texts with zeros and attends over the padding, so an
utterance's GTA mel depends on its batch companions; here every sentence is decoded as if alone (the reference at batch size 1), whatever
--max_batch says.

`--no_kernel` runs the eager loop on whatever torch device there is (a CPU included); without it a HIP device is required.  `--cbhg_kernel` also
runs the encoder and the post-net as HIP kernels.  A sentence of more than 256 ids takes the eager loop on the device."""
import argparse
import pickle
import time
from pathlib import Path

import numpy as np
import torch

from .tacotron import TacotronInference, text_to_ids

CHUNK = 64                     # utterances per forward_gta_batch call (one encoder / post-net call with --cbhg_kernel)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Ground-truth-aligned mels from a reference Tacotron checkpoint on MI355X')
    ap.add_argument('--tts_weights', type=str, required=True, help='[string/path] reference Tacotron state dict (.pyt)')
    ap.add_argument('--path', type=str, required=True, help='the reference\'s data directory: dataset.pkl, text_dict.pkl, mel/<id>.npy')
    ap.add_argument('--out', type=str, default=None, help='output directory (default: <path>/gta)')
    ap.add_argument('--max_batch', type=int, default=8, help='sentences per decoder kernel (1..8)')
    ap.add_argument('--groups', type=int, default=1, choices=[1, 2], help='decoder groups per launch (2: a group on each half of a 256-CU device)')
    ap.add_argument('--cbhg_kernel', action='store_true', help='run the encoder and the post-net as HIP kernels too')
    ap.add_argument('--no_kernel', action='store_true', help='the eager loop on any torch device (no HIP kernel)')
    a = ap.parse_args(argv)
    if not 1 <= a.max_batch <= 8:
        ap.error('--max_batch: 1..8 sentences per decoder kernel')
    if a.no_kernel and a.cbhg_kernel:
        ap.error('--cbhg_kernel needs the kernel path')
    if not a.no_kernel and not torch.cuda.is_available():
        raise SystemExit('the kernel path needs a HIP device (--no_kernel runs the eager loop on the CPU)')
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    tts = TacotronInference(torch.load(a.tts_weights, map_location=dev), device=dev)
    data = Path(a.path)
    with open(data / 'dataset.pkl', 'rb') as f:
        dataset = pickle.load(f)
    with open(data / 'text_dict.pkl', 'rb') as f:
        text_dict = pickle.load(f)
    out_dir = Path(a.out) if a.out else data / 'gta'
    out_dir.mkdir(parents=True, exist_ok=True)
    t0, frames = time.perf_counter(), 0
    for c in range(0, len(dataset), CHUNK):
        items = dataset[c:c + CHUNK]
        mels = [np.load(data / 'mel' / f'{item_id}.npy').astype(np.float32) for item_id, _ in items]
        outs = tts.forward_gta_batch([text_to_ids(text_dict[item_id]) for item_id, _ in items], [m * 8 - 4 for m in mels],
                                     kernel=not a.no_kernel, cbhg_kernel=a.cbhg_kernel, max_batch=a.max_batch, groups=a.groups)
        for (item_id, _), m, (_, gta, _) in zip(items, mels, outs):               # `_, gta, _ = model(x, mels)` (:187)
            N = m.shape[1]
            np.save(out_dir / f'{item_id}.npy', ((gta[:, :N] + 4) / 8).astype(np.float32), allow_pickle=False)
            frames += N
        print(f'{min(c + CHUNK, len(dataset))}/{len(dataset)} utterances')
    dt = time.perf_counter() - t0
    print(f'{len(dataset)} utterances, {frames} frames in {dt:.1f} s ({len(dataset) / max(dt, 1e-9):.1f} utterances/s) -> {out_dir}')


if __name__ == '__main__':
    main()
