"""`python -m wavernn_amd.score_wavernn --weights W.pyt --mels DIR --wavs DIR` -- the teacher-forced negative log-likelihood a checkpoint gives
to a corpus (score.py): what the reference's validation would report with its training loss (train_wavernn.py:83, :123), on the loop kernels.

DIR/<id>.npy mels (80, N) in [0, 1] are paired by <id> with DIR/<id>.npy (a float waveform in [-1, 1], or integer labels as preprocess.py writes
them) or DIR/<id>.wav (16-bit PCM) audio ALREADY at the model's sample rate -- nothing is resampled.  One line per utterance, then the corpus mean
over all counted samples.

The reference trains its vocoder on ground-truth-aligned mels, not on the recordings' own: `--mels DATA/gta --wavs DATA/quant` (DATA/gta as
`python -m wavernn_amd.gta_tacotron --tts_weights T.pyt --path DATA` or the reference's `train_tacotron.py --force_gta` writes it) scores the vocoder
against what it was trained on."""
import argparse
from pathlib import Path

import numpy as np
import torch

from ._lib import ALGOS
from .model import WaveRNN
from .synthetic import SHIPPED


def load_audio(path: Path, sample_rate):
    if path.suffix == '.npy':
        return np.load(path)
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if sr != sample_rate:
        raise ValueError(f'{path}: {sr} Hz, the model runs at {sample_rate} Hz (nothing is resampled here)')
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError(f'{path}: expected 16-bit mono PCM, got {x.dtype} {x.shape}')
    return (x.astype(np.float32) / np.float32(32768)).clip(-1, 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Score audio under a WaveRNN model on MI355X (teacher-forced NLL)')
    ap.add_argument('--weights', '-w', type=str, help='state-dict .pyt of the reference WaveRNN (random init if omitted)')
    ap.add_argument('--mels', required=True, help='directory of <id>.npy mel spectrograms (80, N) in [0, 1]')
    ap.add_argument('--wavs', required=True, help='directory of <id>.npy or <id>.wav audio at the model sample rate')
    ap.add_argument('--mode', default='MOL', choices=['MOL', 'RAW'])
    ap.add_argument('--mu_law', action='store_true', help='RAW: mu-law encode the waveform (hparams.mu_law) instead of linear labels')
    ap.add_argument('--tile-width', type=int, default=0, choices=[0, 2, 4, 8], help="with --algo tile: workgroups per tile of 16 segments "
                        "(model.tile_width; wrnn_tile_wide_kernel, the same samples bit for bit).  0 (default): wrnn_tile_kernel.  Any other --algo refuses it")
    ap.add_argument('--algo', default='auto', choices=sorted(ALGOS), help="the loop kernel (model.loop_algo); 'tile_sparse' scores a pruned model of other dims than the shipped ones on its surviving 16x1 blocks: "
                         "it needs rnn_dims % 16 == 0 and GRU matrices of which at most 41 % of the blocks survive (sparsity >= 0.6); "
                         "'tile_bf16' scores such a model with its weights rounded to bfloat16: against --algo tile that is what the rounding costs, in bits per sample")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('wavernn_amd needs a HIP device; there is no CPU path (use the reference for that)')
    model = WaveRNN(**SHIPPED, mode=a.mode).to('cuda')
    if a.weights:
        model.load(a.weights)
    model.loop_algo = a.algo
    model.tile_width = a.tile_width
    wav_dir, ids, mels, wavs = Path(a.wavs), [], [], []
    for mel_path in sorted(Path(a.mels).glob('*.npy')):
        audio = next((wav_dir / (mel_path.stem + ext) for ext in ('.npy', '.wav') if (wav_dir / (mel_path.stem + ext)).exists()), None)
        if audio is None:
            raise SystemExit(f'no audio for {mel_path.name} in {wav_dir}')
        mel = np.load(mel_path)
        if mel.ndim != 2 or mel.shape[0] != 80:
            raise ValueError(f'Expected a numpy array shaped (n_mels, n_hops), but got {mel.shape}!')
        ids.append(mel_path.stem)
        mels.append(torch.tensor(mel, dtype=torch.float32).unsqueeze(0))
        wavs.append(load_audio(audio, model.sample_rate))
    if not ids:
        raise SystemExit(f'no .npy mels in {a.mels}')
    from .batch import score_corpus
    res = score_corpus(model, mels, wavs, mu_law=a.mu_law)
    for i, r in zip(ids, res):
        print(f'{i}: {r["steps"]} samples, nll {r["nll_mean"]:.6f} nats/sample = {r["bits_per_sample"]:.6f} bits/sample')
    total, steps = sum(r['nll_sum'] for r in res), sum(r['steps'] for r in res)
    print(f'corpus: {len(ids)} utterances, {steps} samples, nll {total / steps:.6f} nats/sample = {total / steps / np.log(2):.6f} bits/sample '
          f'({model.last_loop_kernel})')


if __name__ == '__main__':
    main()
