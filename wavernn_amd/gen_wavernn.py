"""`python -m wavernn_amd.gen_wavernn --file mel.npy --weights latest_weights.pyt` -- the `--file x.npy` path of the
reference's vocoder CLI (gen_wavernn.py:38-65, :68-142) on the MI355X-native generate path (`--file x.wav` goes through the
librosa-free mel front-end of dsp.py).

Same flags as the reference where they exist (--batched/-b, --unbatched/-u, --target/-t, --overlap/-o, --file/-f,
--weights/-w); the hparams.py machinery is replaced by flags with the shipped defaults (hparams.py:20-60).  Mel
input must be a (80, N) or (1, 80, N) float array in [0, 1] (gen_wavernn.py:50-55 raises ValueError otherwise).

`--unbatched --stream`: the same file through `WaveRNN.generate_stream` -- the audio leaves the device in chunks of --chunk-steps loop steps while the
loop goes on; the time to the first chunk is printed."""
import argparse
from pathlib import Path

import numpy as np
import torch

from ._lib import ALGOS
from .model import WaveRNN
from .synthetic import SHIPPED


def gen_from_file(model, load_path: Path, save_path: Path, batched, target, overlap, mu_law=True, stream_steps=None, live=False):
    """gen_wavernn.py:38-65 for a `.npy` mel."""
    suffix = load_path.suffix
    if suffix == '.wav':
        # gen_wavernn.py:44-47: the librosa front-end, restated without librosa (dsp.py; parity unpinned -- see its header)
        from . import dsp
        wav = dsp.load_wav(load_path, model.sample_rate)
        dsp.save_wav(wav, save_path / f'__{load_path.stem}__{model.get_step() // 1000}k_steps_target.wav', model.sample_rate)
        mel = dsp.melspectrogram(wav)
    elif suffix == '.npy':
        mel = np.load(load_path)
        if mel.ndim != 2 or mel.shape[0] != 80:
            raise ValueError(f'Expected a numpy array shaped (n_mels, n_hops), but got {mel.shape}!')
        _max, _min = mel.max(), mel.min()
        if _max >= 1.01 or _min <= -0.01:
            raise ValueError(f'Expected spectrogram range in [0,1] but was instead [{_min}, {_max}]')
    else:
        raise ValueError(f'Expected an extension of .wav or .npy, but got {suffix}!')
    mel = torch.tensor(mel).unsqueeze(0)
    batch_str = f'gen_batched_target{target}_overlap{overlap}' if batched else 'gen_NOT_BATCHED'
    save_str = save_path / f'__{load_path.stem}__{batch_str}.wav'
    if stream_steps is not None:        # (unbatched: the chunks of generate_stream, concatenated, are what generate returns)
        import time
        from .dsp import save_wav
        t0, chunks, first = time.perf_counter(), [], None
        for c in model.generate_stream(mel, mu_law, chunk_steps=stream_steps, live=live):
            first = first if first is not None else time.perf_counter() - t0
            chunks.append(c)
        out = np.concatenate(chunks)
        print(f'first chunk ({len(chunks[0])} samples) after {first * 1e3:.1f} ms, {len(chunks)} chunks in {(time.perf_counter() - t0) * 1e3:.1f} ms')
        save_wav(out, save_str, model.sample_rate)
        return out, save_str
    out = model.generate(mel, save_str, batched, target, overlap, mu_law)
    return out, save_str


def main(argv=None):
    ap = argparse.ArgumentParser(description='Generate WaveRNN samples on MI355X')
    ap.add_argument('--batched', '-b', dest='batched', action='store_true')
    ap.add_argument('--unbatched', '-u', dest='batched', action='store_false')
    ap.add_argument('--target', '-t', type=int, default=11000)
    ap.add_argument('--overlap', '-o', type=int, default=550)
    ap.add_argument('--file', '-f', type=str, required=True, help='.npy mel spectrogram (80, N) in [0,1], or a .wav at the model sample rate')
    ap.add_argument('--weights', '-w', type=str, help='state-dict .pyt of the reference WaveRNN (random init if omitted)')
    ap.add_argument('--mode', default='MOL', choices=['MOL', 'RAW'])
    ap.add_argument('--output', default='.', help='output directory')
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--device-noise', action='store_true', help='draw sampling noise on the GPU (not comparable with a CPU run); the same as --noise device')
    ap.add_argument('--noise', choices=['cpu', 'device', 'library'], default=None,
                    help="cpu (default): the reference's CPU stream after torch.manual_seed(--seed); device: torch's device generator; library: drawn inside "
                         'the loop from a counter-based generator -- the utterance sounds the same alone and in any gen_corpus batch with the same seed')
    ap.add_argument('--tile-width', type=int, default=0, choices=[0, 2, 4, 8], help="with --algo tile: workgroups per tile of 16 segments "
                        "(model.tile_width; wrnn_tile_wide_kernel, the same samples bit for bit).  0 (default): wrnn_tile_kernel.  Any other --algo refuses it")
    ap.add_argument('--algo', default='auto', choices=sorted(ALGOS),
                    help="the loop kernel (model.loop_algo; WRNN_ALGO_* of include/wavernn_amd.h).  auto (default): the library picks; a kernel by name runs or "
                         "says what it needs -- 'tile' takes models with other dims than the shipped ones, 16 segments per workgroup; 'tile_sparse' is 'tile' for a PRUNED "
                         "such model: it needs rnn_dims % 16 == 0 and GRU matrices of which at most 41 % of the 16x1 blocks survive (sparsity >= 0.6), and skips the pruned ones; "
                         "'tile_bf16' is 'tile' with the weights rounded to bfloat16 on the bf16 matrix pipe -- not the reference's arithmetic")
    ap.add_argument('--stream', action='store_true', help='--unbatched: hand the audio on in chunks while the loop goes on (WaveRNN.generate_stream); prints the time to the first chunk')
    ap.add_argument('--chunk-steps', type=int, default=2200, help='--stream: loop steps per chunk')
    ap.add_argument('--live', action='store_true', help='--stream on a loop kernel that is launched once for all steps (models of non-shipped dims; --algo tile*): '
                        'the call runs whole, publishes its progress, and the chunks leave while it runs (generate_stream(live=True)).  No effect without --stream, '
                        'nor on the shipped dims this tool builds its model with: their kernels continue a call and stream in step slices anyway')
    ap.set_defaults(batched=True)
    a = ap.parse_args(argv)
    if a.stream and a.batched:
        ap.error('--stream needs --unbatched (a folded utterance is finished by its cross-fade, not step by step)')
    if a.chunk_steps < 1:
        ap.error('--chunk-steps: at least one step')
    if not torch.cuda.is_available():
        raise SystemExit('wavernn_amd needs a HIP device; there is no CPU path (use the reference for that)')
    model = WaveRNN(**SHIPPED, mode=a.mode).to('cuda')
    if a.weights:
        model.load(a.weights)
    if a.device_noise and a.noise not in (None, 'device'):
        ap.error('--device-noise contradicts --noise ' + a.noise)
    model.noise_source = 'device' if a.device_noise else (a.noise or 'cpu')
    model.loop_algo = a.algo
    model.tile_width = a.tile_width
    if a.seed is not None:
        torch.manual_seed(a.seed)
        model.noise_seed = a.seed
    out, path = gen_from_file(model, Path(a.file).expanduser().resolve(), Path(a.output), a.batched, a.target, a.overlap,
                              stream_steps=a.chunk_steps if a.stream else None, live=a.live)
    n = out.shape[0]
    print(f'{path}: {n} samples ({n / model.sample_rate:.2f} s), loop {model.last_loop_kernel} {model.last_loop_ms:.1f} ms '
          f'= {n / model.last_loop_ms:.1f} kHz')


if __name__ == '__main__':
    main()
