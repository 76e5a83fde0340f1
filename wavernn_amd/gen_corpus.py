"""Batch vocoding of a directory of mel spectrograms on one or several GPUs (BASELINE config 4).

    python -m wavernn_amd.gen_corpus --mels mels_dir --weights latest_weights.pyt --output wavs
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m wavernn_amd.gen_corpus ...

Every `*.npy` under --mels is a (80, N) mel in [0, 1] (the reference's `gen_wavernn.py --file x.npy` input,
gen_wavernn.py:38-65).  All utterances are folded into one segment table (`batch.plan_utterances`), the table is cut into
one contiguous block per rank, each rank runs ONE loop launch, the finished audio is all-gathered (RCCL) and every rank
writes the WAVs of the utterances whose first segment it owned.  `--seed S` gives utterance u the parity noise stream of
`torch.manual_seed(S + u)` (equal to a per-utterance `generate()` call with that seed); without it noise is drawn on the
device.  `--noise library --seed S`: the loop draws its noise itself, utterance u under seed S + u (equal to
`gen_wavernn --noise library --seed S+u`, whatever the batch and the rank count; no noise crosses the host).

`--unbatched [--chunk-steps K]`: the quality mode -- no folds, no cross-fade seams -- for the whole directory in one pass (`batch.generate_unbatched`:
every utterance one unfolded segment, up to 64 per loop call); single process; files are named `..gen_NOT_BATCHED.wav` as gen_wavernn names them.
With --chunk-steps the audio leaves the device in slices of K steps while the loop goes on.
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from ._lib import ALGOS
from .batch import generate_corpus, generate_unbatched
from .dsp import save_wav
from .model import WaveRNN
from .synthetic import SHIPPED


def load_mels(mel_dir):
    paths = sorted(Path(mel_dir).expanduser().glob('*.npy'))
    if not paths:
        raise ValueError(f'no .npy files under {mel_dir}')
    mels = []
    for p in paths:
        m = np.load(p)
        if m.ndim != 2 or m.shape[0] != 80:
            raise ValueError(f'{p}: expected a numpy array shaped (n_mels, n_hops), but got {m.shape}!')
        if m.max() >= 1.01 or m.min() <= -0.01:
            raise ValueError(f'{p}: expected spectrogram range in [0,1] but was instead [{m.min()}, {m.max()}]')
        if m.shape[1] < 21:
            raise ValueError(f'{p}: {m.shape[1]} frames; the reference needs wave_len >= 20*hop (21 frames)')
        mels.append(torch.from_numpy(m.astype(np.float32)).unsqueeze(0))
    return paths, mels


def main(argv=None):
    ap = argparse.ArgumentParser(description='Vocode a directory of mels with WaveRNN on MI355X (one launch per GPU)')
    ap.add_argument('--mels', required=True, help='directory of (80, N) .npy mel spectrograms')
    ap.add_argument('--weights', '-w', help='state-dict .pyt of the reference WaveRNN (random init if omitted)')
    ap.add_argument('--output', default='model_outputs')
    ap.add_argument('--target', '-t', type=int, default=11000)
    ap.add_argument('--overlap', '-o', type=int, default=550)
    ap.add_argument('--mode', default='MOL', choices=['MOL', 'RAW'])
    ap.add_argument('--seed', type=int, default=None, help='parity noise: utterance u uses torch.manual_seed(seed + u); --noise library: its stream seed')
    ap.add_argument('--noise', choices=['cpu', 'device', 'library'], default=None,
                    help='where the sampling noise comes from (default: cpu with --seed, else device); cpu and library need --seed')
    ap.add_argument('--sparse-groups', type=int, default=None, choices=[1, 2],
                    help='a pruned MoL model on wrnn_sparse_kernel: groups of segments per cluster (2: 512 segments a round; a dense model ignores it)')
    ap.add_argument('--tile-width', type=int, default=0, choices=[0, 2, 4, 8], help="with --algo tile: workgroups per tile of 16 segments "
                        "(model.tile_width; wrnn_tile_wide_kernel, the same samples bit for bit).  0 (default): wrnn_tile_kernel.  Any other --algo refuses it")
    ap.add_argument('--algo', default='auto', choices=sorted(ALGOS),
                    help="the loop kernel (model.loop_algo; WRNN_ALGO_* of include/wavernn_amd.h).  auto (default): the library picks; a kernel by name runs or "
                         "says what it needs -- 'tile' takes models with other dims than the shipped ones, 16 segments per workgroup; 'tile_sparse' is 'tile' for a PRUNED "
                         "such model: it needs rnn_dims % 16 == 0 and GRU matrices of which at most 41 % of the 16x1 blocks survive (sparsity >= 0.6), and skips the pruned ones; "
                         "'tile_bf16' is 'tile' with the weights rounded to bfloat16 on the bf16 matrix pipe -- not the reference's arithmetic")
    ap.add_argument('--unbatched', '-u', action='store_true', help='no folds: every utterance one unfolded segment, up to 64 per loop call (single process)')
    ap.add_argument('--chunk-steps', type=int, default=None, help='--unbatched: finish and copy out the audio in slices of K loop steps while the loop goes on')
    ap.add_argument('--live', action='store_true', help='--unbatched --chunk-steps K on a loop kernel that is launched once for all steps (models of non-shipped dims): the call '
                        'runs whole, publishes its progress, and the chunks leave while it runs (generate_unbatched(live=True)).  No effect without --chunk-steps, nor on the '
                        'shipped dims this tool builds its model with: their kernels continue a call and stream in step slices anyway')
    a = ap.parse_args(argv)
    if a.noise in ('cpu', 'library') and a.seed is None:
        ap.error(f'--noise {a.noise} needs --seed')
    if a.live and not a.unbatched:
        ap.error('--live needs --unbatched')
    if a.chunk_steps is not None and not a.unbatched:
        ap.error('--chunk-steps needs --unbatched')
    if a.chunk_steps is not None and a.chunk_steps < 1:
        ap.error('--chunk-steps: at least one step')
    if a.unbatched and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise SystemExit('gen_corpus --unbatched runs in a single process (an unbatched list is not sharded over ranks); start it without a launcher')
    if not torch.cuda.is_available():
        raise SystemExit('wavernn_amd needs a HIP device; there is no CPU path (use the reference for that)')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    group = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)      # nccl == RCCL on ROCm
        group = dist.group.WORLD
    model = WaveRNN(**SHIPPED, mode=a.mode).to(dev)
    if a.weights:
        model.load(a.weights)
    model.sparse_groups = a.sparse_groups
    model.loop_algo = a.algo
    model.tile_width = a.tile_width
    paths, mels = load_mels(a.mels)
    seeds = [a.seed + u for u in range(len(mels))] if a.seed is not None else None
    noise = a.noise or ('cpu' if seeds is not None else 'device')
    if a.unbatched:
        outs = generate_unbatched(model, [m.to(dev) for m in mels], True, seeds, noise_source=noise, chunk_steps=a.chunk_steps, live=a.live)
    else:
        outs = generate_corpus(model, [m.to(dev) for m in mels], a.target, a.overlap, True, seeds, group=group, noise_source=noise, finish='own')
    out_dir = Path(a.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    n = 0
    for p, y in zip(paths, outs):
        if y is not None:
            batch_str = 'gen_NOT_BATCHED' if a.unbatched else f'gen_batched_target{a.target}_overlap{a.overlap}'
            save_wav(y, out_dir / f'__{p.stem}__{batch_str}.wav', model.sample_rate)
            n += y.shape[0]
    eng = model._loop_engine()
    print(f'rank {rank}/{world}: wrote {sum(y is not None for y in outs)} of {len(outs)} utterances, {n / model.sample_rate:.1f} s of audio; '
          f'loop {eng.last_loop_kernel()} {eng.last_loop_ms():.0f} ms')
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
