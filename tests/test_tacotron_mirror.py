"""`wavernn_amd.tacotron.TacotronInference` (the functional, state-dict-driven restatement of the reference's
`Tacotron.generate()`, BASELINE config 3's caller side) against what the reference class itself returned, on the CPU.
tests/golden/tacotron_mirror.npz holds the reference's outputs (scripts/make_golden.py).  Same weights, same ids -> the same
mel / linear / attention: bit-identical on the host that made the fixture, <= TOL on another host's CPU (torch's CPU kernels
round differently from one processor to the next: ~2e-7 over 800 decoder steps) -- the tolerance of the sibling check
test_oracle_golden.py::test_tacotron_mirror_reproduces_the_reference_decoder_fixture.  Also pinned: the mel committed in
tests/golden/mol_tacotron_800f.npz (the input of config 3's vocoder parity tests)."""
import ast
import json
import os

import numpy as np
import torch

from helpers import GOLDEN, load_case, rich_tacotron_state_dict

TOL = 1e-6


def _close(a, b):
    return a.shape == b.shape and float(np.abs(a - b).max()) <= TOL


def _golden():
    g = np.load(os.path.join(GOLDEN, 'tacotron_mirror.npz'))
    shapes = json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json')))
    wseed = ast.literal_eval(str(g["config"]))['wseed']
    return g, rich_tacotron_state_dict(wseed, shapes), [int(i) for i in g['ids']]


def test_functional_tacotron_equals_the_reference():
    from wavernn_amd.tacotron import TacotronInference, text_to_ids, tacotron_to_wavernn_mel
    g, sd, ids = _golden()
    assert text_to_ids(str(g['line'])) == ids                      # plain text: basic cleaning == the reference's english_cleaners
    mel, lin, attn = TacotronInference(sd).generate(ids, steps=60)
    assert mel.shape == g['mel_r1_60'].shape == (80, 60) and attn.shape == g['attention_r1_60'].shape == (60, len(ids))
    assert _close(mel, g['mel_r1_60']) and _close(lin, g['linear_r1_60']) and _close(attn, g['attention_r1_60'])
    # r > 1 (the reference's progressive schedule trains with r = 7 .. 2): several frames per decoder step
    sd3 = dict(sd, **{'decoder.r': torch.tensor(3, dtype=sd['decoder.r'].dtype)})
    mel3, _, attn3 = TacotronInference(sd3).generate(ids, steps=30)
    assert mel3.shape == g['mel_r3_30'].shape == (80, 30) and _close(mel3, g['mel_r3_30']) and _close(attn3, g['attention_r3_30'])
    assert tacotron_to_wavernn_mel(mel).min() >= 0 and tacotron_to_wavernn_mel(mel).max() <= 1


def test_config3_fixture_mel_links_to_the_mirror_through_the_reference():
    """the mel stored in tests/golden/mol_tacotron_800f.npz is what the reference's gen_tacotron.py hands its vocoder: the
    SECOND return of `Tacotron.generate` (`_, m, attention = tts_model.generate(x)`, gen_tacotron.py:142 -- the postnet /
    post_proj output, 80 bins because fft_bins = hp.num_mels), rescaled and clipped (:143-145).

    The link to the mirror is INDIRECT: the fixture's weights are the reference's torch-initialised `torch.manual_seed(3)` Tacotron
    (11.1 M parameters, not stored), so the mirror does not run on them here.  Two facts are checked instead: (1) the mirror reproduces
    the reference's two returns over the fixture's 800 decoder steps on other weights (rich_tacotron_state_dict, <= TOL); (2) the
    reference's stored second return for the fixture's weights, rescaled, IS the fixture mel, and its first return is not (round-2
    advisor: this test compared the raw decoder mel -- the FIRST return -- and hid the 0.04 difference behind a 0.25 tolerance)."""
    from wavernn_amd.tacotron import TacotronInference, tacotron_to_wavernn_mel
    cfg, fx = load_case('mol_tacotron_800f')
    g, sd, ids = _golden()
    assert ast.literal_eval(str(g["config"]))['fixture_tts_seed'] == cfg['tts_seed']
    mel, lin, _ = TacotronInference(sd).generate(ids, steps=cfg['frames'])
    assert _close(mel, g['mel_r1_800']) and _close(lin, g['linear_r1_800'])
    assert lin.shape == (80, cfg['frames'])
    assert g['fixture_linear'].shape == (80, cfg['frames'])
    assert np.array_equal(tacotron_to_wavernn_mel(g['fixture_linear']).astype(np.float32), fx['mel'])
    assert not np.array_equal(tacotron_to_wavernn_mel(g['fixture_mel']).astype(np.float32), fx['mel'])
