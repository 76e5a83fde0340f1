"""The premise of tests/test_gpu_taco_rich.py, checked on the CPU: on `rich_tacotron_state_dict(5)` and the sentence of
tests/golden/tacotron_mirror.npz at 60 steps, the outputs SEE every bias vector of the model -- so a kernel that reads one of them through a
wrong index, adds it on the wrong side of a gate or drops it for one role cannot stay within that file's bars.

These are conditions on the INPUT (weights and sentence), evaluated on the float32 mirror `TacotronInference.generate`; no kernel is measured
here.  Thresholds: 10 x TACO_TOL for a zeroed vector (the GPU tests' absolute bar is TACO_TOL = 1e-6), 1e-2 for the structural mistakes.
Measured on the mirror: a zeroed vector moves some output by >= 1.06e-5 (`decoder.attn_net.L.bias`, attention; every vector but the two of
the attention net moves mel or linear by >= 9e-4), a roll by one gate block by >= 5e-2, b_hn folded into b_in by >= 3e-2."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, rich_tacotron_state_dict

TACO_TOL = 1e-6                                                          # tests/test_gpu_config3.py
STEPS = 60
SHAPES = json.load(open(os.path.join(GOLDEN, 'tacotron_shapes.json')))
BIASES = [k for k, shape, dtype in SHAPES if dtype == 'float32' and len(shape) == 1 and 'bnorm' not in k and k != 'stop_threshold']
GATE_BIASES = [k for k in BIASES if '.bias_ih' in k or '.bias_hh' in k]
GRUS = ['decoder.attn_rnn.bias_hh', 'encoder.cbhg.rnn.bias_hh_l0', 'encoder.cbhg.rnn.bias_hh_l0_reverse', 'postnet.rnn.bias_hh_l0',
        'postnet.rnn.bias_hh_l0_reverse']


def test_the_model_has_37_bias_vectors():
    assert len(BIASES) == 37 and len(GATE_BIASES) == 14 and set(GRUS) <= set(GATE_BIASES), (len(BIASES), len(GATE_BIASES))
    sd = _state_dict()
    assert all(float(sd[k].abs().min()) > 0 for k in BIASES)             # the rich weights: no bias element is zero


@functools.lru_cache(maxsize=None)
def _state_dict():
    return rich_tacotron_state_dict(5, SHAPES)


@functools.lru_cache(maxsize=None)
def _ids():
    return tuple(int(i) for i in np.load(os.path.join(GOLDEN, 'tacotron_mirror.npz'))['ids'])


def _generate(**override):
    from wavernn_amd.tacotron import TacotronInference
    return TacotronInference(dict(_state_dict(), **override)).generate(list(_ids()), steps=STEPS)


@functools.lru_cache(maxsize=None)
def _baseline():
    """(mel, linear, attention) of the unchanged weights: computed once, shared, never modified."""
    return _generate()


def _moved(**override):
    """max |output of the changed weights - baseline| for (mel, linear, attention)."""
    return [float(np.abs(a - b).max()) for a, b in zip(_generate(**override), _baseline())]


def _blocks(key):
    return 4 if 'res_rnn' in key else 3                                  # LSTM: i, f, g, o; GRU: r, z, n


def test_the_baseline_is_the_fixture():
    g = np.load(os.path.join(GOLDEN, 'tacotron_mirror.npz'))
    for name, mine in zip(('mel', 'linear', 'attention'), _baseline()):
        assert mine.shape == g[f'{name}_r1_60'].shape and float(np.abs(mine - g[f'{name}_r1_60']).max()) <= TACO_TOL, name


@pytest.mark.parametrize('key', BIASES)
def test_zeroing_a_bias_vector_moves_an_output(key):
    d = _moved(**{key: torch.zeros_like(_state_dict()[key])})
    print(f'{key} = 0: mel {d[0]:.3e} linear {d[1]:.3e} attention {d[2]:.3e}')
    assert max(d) >= 10 * TACO_TOL, (key, d)


@pytest.mark.parametrize('key', GATE_BIASES)
def test_rolling_the_gate_blocks_moves_mel_or_linear(key):
    """The vector with its gate blocks rotated by one: what a wrong `q` in `b[q * H + j]` reads."""
    b = _state_dict()[key]
    H = b.numel() // _blocks(key)
    assert H * _blocks(key) == b.numel()
    d = _moved(**{key: torch.roll(b, H)})
    print(f'{key} rolled by {H}: mel {d[0]:.3e} linear {d[1]:.3e} attention {d[2]:.3e}')
    assert max(d[:2]) >= 1e-2, (key, d)


@pytest.mark.parametrize('key', GRUS)
def test_folding_b_hn_into_b_in_moves_mel_or_linear(key):
    """n = tanh(W_in x + b_in + r * (W_hn h + b_hn)): with b_hn moved outside the product (added to b_in, zero inside) r no longer scales it."""
    sd = _state_dict()
    ih_key = key.replace('bias_hh', 'bias_ih')
    b_ih, b_hh = sd[ih_key].clone(), sd[key].clone()
    H = b_hh.numel() // 3
    b_ih[2 * H:] += b_hh[2 * H:]
    b_hh[2 * H:] = 0
    d = _moved(**{key: b_hh, ih_key: b_ih})
    print(f'{key}: b_hn folded into b_in: mel {d[0]:.3e} linear {d[1]:.3e} attention {d[2]:.3e}')
    assert max(d[:2]) >= 1e-2, (key, d)
