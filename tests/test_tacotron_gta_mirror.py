"""`TacotronInference.forward_gta(kernel=False)` on the CPU against what the reference's own `Tacotron.forward(x, m, generate_gta=True)`
(models/tacotron.py:310-368) returned for the same weights, ids and forced mel: tests/golden/tacotron_gta.npz, cases m0 (r = 1, N = 30) and m1
(r = 3, N = 31 -- 11 steps, 33 frames out), written by scripts/make_golden_gta.py for `rich_tacotron_state_dict(5)`.  The bar is the one
tests/test_tacotron_mirror.py holds `generate()` to: the same shapes and max |difference| <= 1e-6 (torch's CPU kernels round differently from one
processor to the next)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, rich_tacotron_state_dict

TOL = 1e-6                                                               # tests/test_tacotron_mirror.py


def _close(a, b):
    return a.shape == b.shape and float(np.abs(a - b).max()) <= TOL


def _tts(r):
    from wavernn_amd.tacotron import TacotronInference
    sd = rich_tacotron_state_dict(5, json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json'))))
    sd = dict(sd, **{'decoder.r': torch.tensor(r, dtype=sd['decoder.r'].dtype)})
    tts = TacotronInference(sd)
    assert tts.r == r
    return tts


@pytest.mark.parametrize('tag', ['m0', 'm1'])
def test_forward_gta_equals_the_reference(tag):
    g = np.load(os.path.join(GOLDEN, 'tacotron_gta.npz'))
    r, ids, force = int(g[f'{tag}_r']), [int(i) for i in g[f'{tag}_ids']], g[f'{tag}_force_mel']
    N = force.shape[1]
    steps = (N + r - 1) // r
    assert (r, N) == {'m0': (1, 30), 'm1': (3, 31)}[tag]
    tts = _tts(r)
    tts.stop_threshold = 1e9                                             # a stop test left in the loop would end the run at the first t > 10 (12 frames)
    gta, lin, attn = tts.forward_gta(ids, force)
    assert gta.shape == (80, steps * r) and lin.shape == (80, steps * r) and attn.shape == (steps, len(ids))
    for name, mine in (('gta', gta), ('linear', lin), ('attention', attn)):
        ref = g[f'{tag}_{name}']
        print(f'{tag} {name}: max |mirror - reference| = {float(np.abs(mine - ref).max()):.3e}')
        assert _close(mine, ref), name
    # teacher forcing is what is checked: the free-running decoder is far from this (0.58 / 0.70 for these weights)
    free, _, _ = _tts(r).generate(ids, steps=N)
    assert float(np.abs(free[:, :N] - gta[:, :N]).max()) > 0.1


def test_forward_gta_accepts_tensors_and_rejects_an_empty_mel():
    g = np.load(os.path.join(GOLDEN, 'tacotron_gta.npz'))
    tts = _tts(1)
    ids, force = [int(i) for i in g['m0_ids']], g['m0_force_mel'][:, :3]
    a = tts.forward_gta(ids, force)
    b = tts.forward_gta(ids, torch.from_numpy(force).unsqueeze(0))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].shape == (80, 3)
    assert _close(a[0], g['m0_gta'][:, :3])                              # causal: the first frames do not depend on the later ones
    with pytest.raises(ValueError):
        tts.forward_gta(ids, np.zeros((80, 0), np.float32))
