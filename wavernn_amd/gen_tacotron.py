"""`python -m wavernn_amd.gen_tacotron --input_text "..." --tts_weights tts.pyt --voc_weights voc.pyt` -- the `wavernn` vocoder
path of the reference's TTS CLI (gen_tacotron.py:97-166) on one MI355X: Tacotron (functional PyTorch-ROCm restatement with a
the decoder loop as one persistent HIP kernel, `tacotron.py` / csrc/wrnn_taco.hip; `_, m, attention = tts_model.generate(x)` :142 -- the vocoder is fed the SECOND return,
the postnet / post_proj output, 80 bins because fft_bins = hp.num_mels) -> (m + 4) / 8, clip (:143-145) -> the MI355X-native `WaveRNN.generate` (:161-163).

Flags follow the reference where they exist (--input_text/-i, --tts_weights, --batched/-b, --unbatched/-u, --target/-t,
--overlap/-o, --voc_weights); hparams.py is replaced by the shipped defaults.  Without --input_text every line of
--sentences (default: none) is synthesised.  Text cleaning is the basic pipeline (lowercase, whitespace): number and
abbreviation expansion need the reference's text front-end (out of scope).

`--batch N`: all sentences at once -- the Tacotron decoder loops in groups of N <= 8 sentences per persistent kernel
(`TacotronInference.generate_batch`, csrc/wrnn_taco_batch.hip), then ONE vocoder pass over all of them (`generate_corpus`, noise drawn inside the
library under the seeds --seed, --seed + 1, ...).  Same file names.  With --cbhg_kernel the encoder and the post-net of all sentences run side by
side as well (`wrnn_taco_encode_many` / `wrnn_taco_postnet_many`, one call each per 64 sentences).  Without the flag the per-sentence path runs as
before.  `--groups 2` (with --batch, a device of 256 CUs): two decoder groups of N sentences per launch, one on each half of the device
(`wrnn_taco_decode_batch_groups`); the same audio.  `--batch N --unbatched`: the same Tacotron side, and the vocoder pass is
`generate_unbatched` -- every sentence one unfolded segment of one loop call, no folds and no cross-fade seams, the same seeds."""
import argparse
import time
from pathlib import Path

import numpy as np
import torch

from .model import WaveRNN
from .synthetic import SHIPPED
from .tacotron import TacotronInference, tacotron_to_wavernn_mel, text_to_ids


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='TTS Generator (Tacotron -> WaveRNN) on MI355X')
    ap.add_argument('--input_text', '-i', type=str, help='[string] Type in something here and TTS will generate it!')
    ap.add_argument('--sentences', type=str, help='text file, one sentence per line (the reference reads sentences.txt)')
    ap.add_argument('--tts_weights', type=str, required=True, help='[string/path] reference Tacotron state dict (.pyt)')
    ap.add_argument('--voc_weights', type=str, required=True, help='[string/path] reference WaveRNN state dict (.pyt)')
    ap.add_argument('--batched', '-b', dest='batched', action='store_true')
    ap.add_argument('--unbatched', '-u', dest='batched', action='store_false')
    ap.add_argument('--target', '-t', type=int, default=11_000)
    ap.add_argument('--overlap', '-o', type=int, default=550)
    ap.add_argument('--mode', default='MOL', choices=['MOL', 'RAW'])
    ap.add_argument('--steps', type=int, default=2000, help='decoder step limit (Tacotron.generate default)')
    ap.add_argument('--output', default='.', help='output directory')
    ap.add_argument('--cbhg_kernel', action='store_true', help='run the encoder and the post-net as HIP kernels too (wrnn_taco_encode / wrnn_taco_postnet; with --batch their _many forms)')
    ap.add_argument('--batch', type=int, default=None, help='decode up to N (1..8) sentences per Tacotron kernel and vocode them in one pass (--unbatched: unfolded, generate_unbatched)')
    ap.add_argument('--groups', type=int, default=1, choices=[1, 2], help='--batch: decoder groups per launch (2: a group on each half of a 256-CU device)')
    ap.add_argument('--seed', type=int, default=0, help='--batch: sentence i draws its sampling noise under seed + i')
    ap.add_argument('--live', action='store_true', help='--batch N --unbatched: passed on to generate_unbatched(live=True).  No effect here: this tool asks for no chunks '
                        '(every sentence is written when the pass has ended), and the shipped dims it builds its vocoder with run on kernels that continue a call')
    ap.set_defaults(batched=True)
    a = ap.parse_args(argv)
    if a.batch is not None and not 1 <= a.batch <= 8:
        ap.error('--batch: 1..8 sentences per decoder kernel')
    if a.live and (a.batch is None or a.batched):
        ap.error('--live needs --batch N --unbatched')
    if a.groups != 1 and a.batch is None:
        ap.error('--groups needs --batch')
    return a


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('wavernn_amd needs a HIP device; there is no CPU path (use the reference for that)')
    voc = WaveRNN(**SHIPPED, mode=a.mode).to('cuda')
    voc.load(a.voc_weights)
    tts = TacotronInference(torch.load(a.tts_weights, map_location='cuda'), device='cuda')
    if a.input_text:
        texts = [a.input_text.strip()]
    elif a.sentences:
        texts = [ln.strip() for ln in open(a.sentences) if ln.strip()]
    else:
        raise SystemExit('give --input_text or --sentences')
    out_dir = Path(a.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    v_type = 'wavernn_batched' if a.batched else 'wavernn_unbatched'
    tts_k = int(tts.p['step'].item()) // 1000 if 'step' in tts.p else 0
    names = [f'__input_{text[:10]}_{v_type}_{tts_k}k.wav' if a.input_text else f'{i}_{v_type}_{tts_k}k.wav' for i, text in enumerate(texts, 1)]
    if a.batch is not None:
        from .batch import generate_corpus, generate_unbatched
        from .dsp import save_wav
        print(f'\n| Generating {len(texts)} sentences, {a.batch} per decoder kernel')
        t0 = time.perf_counter()
        outs = tts.generate_batch([text_to_ids(t) for t in texts], steps=a.steps, kernel=True, cbhg_kernel=a.cbhg_kernel, max_batch=a.batch, groups=a.groups)
        t1 = time.perf_counter()
        mels = [torch.tensor(tacotron_to_wavernn_mel(lin)).unsqueeze(0) for _, lin, _ in outs]          # the POSTNET output (:142)
        seeds = [a.seed + i for i in range(len(mels))]
        if a.batched:
            wavs = generate_corpus(voc, mels, a.target, a.overlap, True, seeds=seeds, noise_source='library')
        else:
            wavs = generate_unbatched(voc, mels, True, seeds=seeds, noise_source='library', live=a.live)
        t2 = time.perf_counter()
        for name, wav, (_, lin, _) in zip(names, wavs, outs):
            save_wav(np.asarray(wav), out_dir / name, voc.sample_rate)
            print(f'{name}: {lin.shape[1]} frames, {len(wav) / voc.sample_rate:.2f} s of audio')
        print(f'Tacotron {(t1 - t0) * 1e3:.0f} ms, vocoder {(t2 - t1) * 1e3:.0f} ms for {len(texts)} sentences')
        print('\n\nDone.\n')
        return
    for i, text in enumerate(texts, 1):
        print(f'\n| Generating {i}/{len(texts)}')
        t0 = time.perf_counter()
        _, mel, _ = tts.generate(text_to_ids(text), steps=a.steps, kernel=True, cbhg_kernel=a.cbhg_kernel)   # the POSTNET output (:142)
        t1 = time.perf_counter()
        m = torch.tensor(tacotron_to_wavernn_mel(mel)).unsqueeze(0)
        name = names[i - 1]
        wav = voc.generate(m, out_dir / name, a.batched, a.target, a.overlap, True)
        t2 = time.perf_counter()
        print(f'{name}: {mel.shape[1]} frames, {wav.shape[0] / voc.sample_rate:.2f} s of audio; Tacotron {(t1 - t0) * 1e3:.0f} ms, '
              f'vocoder {(t2 - t1) * 1e3:.0f} ms ({voc.last_loop_kernel})')
    print('\n\nDone.\n')


if __name__ == '__main__':
    main()
