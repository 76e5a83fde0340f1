"""Generate tests/golden/tacotron_gta.npz by RUNNING THE REFERENCE ITSELF (CPU): what its own `Tacotron.forward(x, m, generate_gta=True)`
(models/tacotron.py:310-368) returns -- the teacher-forced decoder over a given mel, in eval mode, at batch size 1.

The fixture of the ground-truth-aligned path (`TacotronInference.forward_gta`, `wrnn_taco_decode_forced`).  Like scripts/make_golden_score.py this
runs only where the reference checkout is mounted (WRNN_REFERENCE, read-only), with the same shims -- a stub `librosa`, `np.cumproduct`, `hparams`
configured, stub `unidecode` / `inflect` --, writes nothing into the reference tree, and the .npz file (arrays only) is committed.

Cases (text, r, N); the forced mel is `random_mel(500 + N, N) * 8 - 4` and is stored:
  the GPU suite's weights `random_tacotron_state_dict(3, shapes)`:  g0 (B, 1, 40)  g1 (A, 1, 23)  g2 (C, 1, 16)  g3 (B, 2, 37)  g4 (A, 1, 1)
  the mirror's weights `rich_tacotron_state_dict(5)` (tests/helpers.py):  m0 (B, 1, 30)  m1 (B, 3, 31)
A = 'Hello there.', B = the suite's 74-id CERN sentence, C = B three times (224 ids).  Per case: ids, force_mel, gta, linear, attention.

    python scripts/make_golden_gta.py
"""
import json, os, sys, types
import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
REF = os.environ.get('WRNN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
lib = types.ModuleType('librosa'); lib.output = types.SimpleNamespace(write_wav=lambda *a, **k: None)
sys.modules['librosa'] = lib
un = types.ModuleType('unidecode'); un.unidecode = lambda s: s
sys.modules.setdefault('unidecode', un)
inf = types.ModuleType('inflect'); inf.engine = lambda: types.SimpleNamespace(number_to_words=lambda *a, **k: 'number')
sys.modules.setdefault('inflect', inf)
if not hasattr(np, 'cumproduct'):
    np.cumproduct = np.cumprod
import torch
from utils import hparams as hp
hp.configure(os.path.join(REF, 'hparams.py'))
from models.tacotron import Tacotron                 # the reference implementation
from utils.text import text_to_sequence
from utils.text.symbols import symbols

from helpers import rich_tacotron_state_dict
from wavernn_amd.synthetic import random_mel, random_tacotron_state_dict
from wavernn_amd.tacotron import text_to_ids

OUT = os.path.join(REPO, 'tests', 'golden')
A_TEXT = 'Hello there.'
B_TEXT = 'Scientists at the CERN laboratory say they have discovered a new particle.'
C_TEXT = ' '.join([B_TEXT] * 3)
GPU_CASES = ((B_TEXT, 1, 40), (A_TEXT, 1, 23), (C_TEXT, 1, 16), (B_TEXT, 2, 37), (A_TEXT, 1, 1))
MIRROR_CASES = ((B_TEXT, 1, 30), (B_TEXT, 3, 31))


def reference_tacotron(sd):
    tts = Tacotron(embed_dims=hp.tts_embed_dims, num_chars=len(symbols), encoder_dims=hp.tts_encoder_dims,
                   decoder_dims=hp.tts_decoder_dims, n_mels=hp.num_mels, fft_bins=hp.num_mels, postnet_dims=hp.tts_postnet_dims,
                   encoder_K=hp.tts_encoder_K, lstm_dims=hp.tts_lstm_dims, postnet_K=hp.tts_postnet_K,
                   num_highways=hp.tts_num_highways, dropout=hp.tts_dropout, stop_threshold=hp.tts_stop_threshold)
    tts.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in sd.items()}, strict=True)
    return tts


def run(tts, out, tag, text, r, N):
    ids = text_to_ids(text)
    assert ids == text_to_sequence(text, hp.tts_cleaner_names)[:len(ids)] and len(text_to_sequence(text, hp.tts_cleaner_names)) in (len(ids), len(ids) + 1)
    force = (random_mel(500 + N, N) * 8 - 4).astype(np.float32)
    tts.r = r
    x, m = torch.as_tensor(ids, dtype=torch.long).unsqueeze(0), torch.from_numpy(force).unsqueeze(0)
    with torch.no_grad():
        gta, lin, attn = tts(x, m, generate_gta=True)
        again = tts(x, m, generate_gta=True)
        free, _, _ = tts.generate(ids, steps=N)
    assert all(torch.equal(a, b) for a, b in zip((gta, lin, attn), again)), 'the call is deterministic'
    steps = (N + r - 1) // r
    assert gta.shape == (1, 80, steps * r) and lin.shape == (1, 80, steps * r) and attn.shape == (1, steps, len(ids)), (gta.shape, lin.shape, attn.shape)
    k = min(gta.shape[2], free.shape[1])
    print(f'{tag}: {len(ids)} ids, r = {r}, N = {N}: gta {tuple(gta.shape)} attention {tuple(attn.shape)}; '
          f'max |forced - free-running| over {k} frames = {float(np.abs(gta[0, :, :k].numpy() - free[:, :k]).max()):.3f}')
    out.update({f'{tag}_ids': np.array(ids, np.int32), f'{tag}_r': np.int32(r), f'{tag}_force_mel': force, f'{tag}_gta': gta[0].numpy(),
                f'{tag}_linear': lin[0].numpy(), f'{tag}_attention': attn[0].numpy()})


def main():
    shapes = json.load(open(os.path.join(OUT, 'tacotron_shapes.json')))
    out = {}
    tts = reference_tacotron(random_tacotron_state_dict(3, shapes))
    for i, c in enumerate(GPU_CASES):
        run(tts, out, f'g{i}', *c)
    tts = reference_tacotron(rich_tacotron_state_dict(5, shapes))
    for i, c in enumerate(MIRROR_CASES):
        run(tts, out, f'm{i}', *c)
    path = os.path.join(OUT, 'tacotron_gta.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 400_000


if __name__ == '__main__':
    main()
