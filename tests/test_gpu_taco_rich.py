"""The Tacotron decoder kernels on weights with NON-ZERO biases (-m gpu): `wrnn_taco_decode` (both variants), `wrnn_taco_decode_batch`,
`wrnn_taco_decode_forced` and the two `_groups` entry points on `helpers.rich_tacotron_state_dict(5)` -- all 37 bias vectors random in
+-0.1 and random batch norms -- against what the REFERENCE's own `Tacotron.generate` / `Tacotron.forward(generate_gta=True)` returned for
these weights (tests/golden/tacotron_mirror.npz, tests/golden/tacotron_gta.npz).  Every other GPU test of the Tacotron side runs on
`random_tacotron_state_dict`, whose biases are exactly zero: a wrong gate offset, a bias on the wrong side of r * (W_hn h + b_hn) or a role
predicate that drops a bias passes there.  tests/test_taco_bias_sensitivity.py shows on the CPU that these outputs see every bias vector.

Sentences: F = the fixtures' sentence (74 ids, `B_TEXT` of tests/test_gpu_taco_batch.py), A (12 ids) and C (224 ids) of that file.  F is held
to the fixtures; A and C to the float32 CPU mirror, which tests/test_tacotron_mirror.py pins to the reference on these weights.

Bars, both asserted for every comparison with a fixture or the mirror (`_check`):
 (a) max |kernel - reference| <= TACO_TOL = 1e-6, the suite's bound;
 (b) the yardstick rule of tests/test_gpu_cbhg.py: per output, e_ref is the larger of two float32 errors against the float64 CPU mirror on
     the same input -- the float32 CPU mirror's and the eager torch-op loop's on the device (`kernel=False`) -- and the kernel's error
     against float64 must be <= MARGIN x e_ref (MARGIN = 8: two valid float32 summation orders).  This bar is what sees an element-level
     mix-up in the attention net, which moves attention by a few 1e-6 only.
Against the same sentence decoded by `wrnn_taco_decode(variant=2)` alone, and against the plain call for a grouped launch: `array_equal`.

Measured on an MI355X: the largest max |kernel - reference| and the largest ratio (kernel error / e_ref) per output over the entry point's
cases.  Outputs reach |mel| <= 0.75 (forced) / 0.35 (free), |linear| <= 0.34, attention <= 0.09; e_ref was 0.9 .. 2.8e-7 for mel, 1.5 ..
1.9e-7 for linear and 1.0e-9 .. 2.5e-8 for attention (its device half moves a little from run to run: MIOpen's convolutions).
  entry point                               |kernel - reference|: mel  linear  attention     ratio: mel  linear  attention
  wrnn_taco_decode variant 2 (r1_60, r3_30)                   8.9e-8  1.6e-7    4.7e-9           0.50    1.00       1.40
  wrnn_taco_decode variant 1 (r1_60, r3_30)                   8.9e-8  1.5e-7    5.6e-9           0.60    1.03       1.05
  generate(cbhg_kernel=True) (r1_60)                          7.5e-8  1.8e-7    4.7e-9           0.45    0.33       0.98
  wrnn_taco_decode_batch S = 1, 3, 8: F                       8.9e-8       -    5.6e-9           0.58       -       1.40
  wrnn_taco_decode_batch S = 3, 8: A, C (mirror)              1.5e-7       -    3.0e-8           0.46       -       1.01
  wrnn_taco_decode_forced m0, m1                              1.8e-7  1.5e-7    4.7e-9           0.44    1.19       0.88
  wrnn_taco_decode_forced S = 3, 8: F                         1.9e-7       -    4.7e-9           0.38       -       0.61
  wrnn_taco_decode_forced S = 3, 8: A, C (mirror)             2.1e-7       -    2.2e-8           0.51       -       0.60
  wrnn_taco_decode_batch_groups: F                            7.6e-8       -    5.6e-9           0.42       -       0.98
  wrnn_taco_decode_forced_groups: F                           1.9e-7       -    4.7e-9           0.38       -       0.61
No output needed the exception for an approximate intrinsic: the kernels' gate functions are expf / tanhf and a true division."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import rich_tacotron_state_dict
from test_gpu_taco_batch import A_TEXT, B_TEXT as F_TEXT, C_TEXT, TACO_TOL, _batch, _single, _tts
from test_gpu_taco_gta import _forced, _seeded_mel
from test_gpu_taco_groups import _forced_call, _forced_read, _grouped_free, _plain_free

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 8.0                                                             # tests/test_gpu_cbhg.py
RICH = 'rich'
FRAMES = {1: 60, 3: 30}                                                  # the fixture's cases r1_60 and r3_30
NO_STOP = -1e9                                                           # a threshold no frame is below: every sentence runs all its steps
FORCED_N = {A_TEXT: 23, C_TEXT: 16}                                      # frames of the seeded forced mels (tests/test_gpu_taco_gta.py)
_MEMO = {}


def _ids(text):
    from wavernn_amd.tacotron import text_to_ids
    return text_to_ids(text)


def _golden(name):
    if name not in _MEMO:
        _MEMO[name] = np.load(os.path.join(HERE, 'golden', name + '.npz'))
    return _MEMO[name]


def _fixture(r):
    """The reference's (mel, linear, attention) for F at r: case r1_60 / r3_30."""
    g = _golden('tacotron_mirror')
    assert [int(i) for i in g['ids']] == _ids(F_TEXT) and len(_ids(A_TEXT)) == 12 and len(_ids(C_TEXT)) == 224
    return {k: g[f'{k}_r{r}_{FRAMES[r]}'] for k in ('mel', 'linear', 'attention')}


def _gta_fixture(tag):
    """The reference's teacher-forced case m0 (r = 1, N = 30) / m1 (r = 3, N = 31) for F: (r, forced mel, dict(mel, linear, attention))."""
    g = _golden('tacotron_gta')
    assert [int(i) for i in g[f'{tag}_ids']] == _ids(F_TEXT)
    return int(g[f'{tag}_r']), g[f'{tag}_force_mel'], dict(mel=g[f'{tag}_gta'], linear=g[f'{tag}_linear'], attention=g[f'{tag}_attention'])


def _forced_mel(text):
    return _gta_fixture('m0')[1] if text == F_TEXT else _seeded_mel(FORCED_N[text])


def _cpu_mirror(r, double):
    key = ('cpu', r, double)
    if key not in _MEMO:
        from wavernn_amd.tacotron import TacotronInference
        sd = rich_tacotron_state_dict(5, json.load(open(os.path.join(HERE, 'golden', 'tacotron_shapes.json'))))
        sd['decoder.r'] = torch.tensor(r, dtype=sd['decoder.r'].dtype)
        if double:
            sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        _MEMO[key] = TacotronInference(sd)
        assert _MEMO[key].r == r
    return _MEMO[key]


def _run(tts, text, forced, **kw):
    """dict(mel, linear, attention) of `generate` (free-running, the fixture's frame count) or `forward_gta` (F: the fixture's forced mel of
    this r; A, C: their seeded mels) on `tts`."""
    if forced:
        force = _gta_fixture('m0' if tts.r == 1 else 'm1')[1] if text == F_TEXT else _forced_mel(text)
        out = tts.forward_gta(_ids(text), force, **kw)
    else:
        out = tts.generate(_ids(text), steps=FRAMES[tts.r], **kw)
    return dict(zip(('mel', 'linear', 'attention'), out))


def _references(text, r, forced=False):
    """(float32 CPU mirror, float64 CPU mirror, e_ref) of a sentence: dicts over mel / linear / attention, computed once, shared, never
    modified.  e_ref: per output the larger of the float32 CPU mirror's and the device's eager loop's error against float64."""
    key = ('ref', text, r, forced)
    if key not in _MEMO:
        ref32, ref64 = _run(_cpu_mirror(r, False), text, forced), _run(_cpu_mirror(r, True), text, forced)
        eager = _run(_tts(r, RICH), text, forced, kernel=False)
        assert all(v.dtype == np.float64 for v in ref64.values())
        e_ref = {k: max(float(np.abs(ref32[k] - ref64[k]).max()), float(np.abs(eager[k] - ref64[k]).max())) for k in ref64}
        for v in list(ref32.values()) + list(ref64.values()):
            v.setflags(write=False)
        _MEMO[key] = (ref32, ref64, e_ref)
    return _MEMO[key]


def _check(what, got, text, r, forced=False, fixture=None):
    """Bars (a) and (b) for the outputs in `got` (a dict over some of mel / linear / attention): (a) against `fixture` (F) or the float32 CPU
    mirror (A, C), (b) against the float64 CPU mirror.  Every figure is printed before anything is asserted."""
    ref32, ref64, e_ref = _references(text, r, forced)
    held_to, word = (fixture, 'fixture') if fixture is not None else (ref32, 'mirror')
    bad = []
    for k, v in got.items():
        assert v.shape == held_to[k].shape == ref64[k].shape, (what, k, v.shape, held_to[k].shape)
        d = float(np.abs(v - held_to[k]).max())
        err = float(np.abs(v.astype(np.float64) - ref64[k]).max())
        ratio = err / e_ref[k]
        print(f'{what} {k}: max |kernel - {word}| = {d:.3e}; max |kernel - f64| = {err:.3e}, e_ref = {e_ref[k]:.3e}, ratio = {ratio:.2f} '
              f'(|x| <= {np.abs(ref64[k]).max():.2f})')
        if not d <= TACO_TOL:
            bad.append((k, 'a', d))
        if not err <= MARGIN * e_ref[k]:
            bad.append((k, 'b', err, e_ref[k], ratio))
    assert not bad, (what, bad)


def _frames(mel):
    """[steps][80][r] as the kernels write it -> (80, steps r), as the reference returns it."""
    return np.ascontiguousarray(mel.transpose(1, 0, 2)).reshape(80, -1)


def _name(text):
    return {F_TEXT: 'F', A_TEXT: 'A', C_TEXT: 'C'}[text]


# ---- wrnn_taco_decode ----
@pytest.mark.parametrize('r', [1, 3])
@pytest.mark.parametrize('variant', [2, 1], ids=['resident', 'flag-barrier'])
def test_single_decode_matches_the_reference(variant, r):
    """`generate(F, kernel=True, kernel_variant=v)` at r1_60 and r3_30: mel and attention out of `wrnn_taco_decode`, and linear out of the torch-op
    post-net with `wrnn_bigru` (the post-net GRU's non-zero b_hh), against the fixture."""
    tts = _tts(r, RICH)
    got = _run(tts, F_TEXT, False, kernel=True, kernel_variant=variant)
    assert tts.last_front_path == 'torch' and got['mel'].shape == (80, FRAMES[r]) and got['attention'].shape == (FRAMES[r] // r, 74)
    _check(f'wrnn_taco_decode variant {variant} r={r} F', got, F_TEXT, r, fixture=_fixture(r))


def test_generate_with_cbhg_kernel_matches_the_reference():
    """End to end through the C ABI on the rich weights: `wrnn_taco_encode` -> `wrnn_taco_decode` -> `wrnn_taco_postnet` against r1_60."""
    tts = _tts(1, RICH)
    got = _run(tts, F_TEXT, False, kernel=True, cbhg_kernel=True)
    assert tts.last_front_path == 'hip'
    _check('generate(cbhg_kernel=True) F', got, F_TEXT, 1, fixture=_fixture(1))


# ---- wrnn_taco_decode_batch ----
BATCHES = {1: [F_TEXT], 3: [A_TEXT, F_TEXT, C_TEXT], 8: [C_TEXT, A_TEXT, A_TEXT, C_TEXT, A_TEXT, F_TEXT, C_TEXT, A_TEXT]}


@pytest.mark.parametrize('r', [1, 3])
@pytest.mark.parametrize('S', [1, 3, 8])
def test_batch_decode_matches_the_reference_and_the_single_kernel(S, r):
    """The <2>, <4> and <8> (LEAN) instantiations, F at another position in each list: F against the fixture, A and C against the CPU mirror,
    and every sentence `array_equal` to `wrnn_taco_decode(variant=2)` of it alone."""
    texts, steps = BATCHES[S], FRAMES[r] // r
    outs = _batch(texts, (steps,) * S, NO_STOP, r, RICH)
    assert len(outs) == S and [k for _, _, k in outs] == [steps] * S
    for s, (text, (mel, sc, k)) in enumerate(zip(texts, outs)):
        mel1, sc1, k1 = _single(text, steps, NO_STOP, r, RICH)
        assert k1 == steps and np.array_equal(mel, mel1) and np.array_equal(sc, sc1), (s, _name(text))
    for s in sorted({texts.index(t) for t in texts}):                    # (equal bits: one check per distinct sentence)
        text, (mel, sc, _) = texts[s], outs[s]
        _check(f'wrnn_taco_decode_batch S={S} r={r} sentence {s} ({_name(text)})', dict(mel=_frames(mel), attention=sc), text, r,
               fixture=_fixture(r) if text == F_TEXT else None)


# ---- wrnn_taco_decode_forced ----
@pytest.mark.parametrize('tag', ['m0', 'm1'])
def test_forced_decode_matches_the_reference(tag):
    """`forward_gta(F, force, kernel=True)`: the pre-pass (the PreNet biases) and the <2, forced> instantiation; m1 at r = 3 over 31 frames."""
    r, force, fixture = _gta_fixture(tag)
    assert (r, force.shape) == {'m0': (1, (80, 30)), 'm1': (3, (80, 31))}[tag]
    got = _run(_tts(r, RICH), F_TEXT, True, kernel=True)
    _check(f'wrnn_taco_decode_forced {tag} r={r} F', got, F_TEXT, r, forced=True, fixture=fixture)


FORCED_BATCHES = {3: [A_TEXT, F_TEXT, C_TEXT], 8: [C_TEXT, A_TEXT, A_TEXT, C_TEXT, F_TEXT, A_TEXT, C_TEXT, A_TEXT]}


@pytest.mark.parametrize('S', [3, 8])
def test_forced_batch_matches_the_reference(S):
    """Forced batches of 3 and 8 (LEAN) at r = 1: F over m0's mel against the fixture, A / 23 and C / 16 over seeded mels against the CPU
    mirror's `forward_gta(kernel=False)`."""
    texts = FORCED_BATCHES[S]
    outs = _forced(texts, [_forced_mel(t) for t in texts], 1, RICH)
    first = {t: texts.index(t) for t in texts}
    for s, (text, (mel, sc)) in enumerate(zip(texts, outs)):
        assert np.array_equal(mel, outs[first[text]][0]) and np.array_equal(sc, outs[first[text]][1]), (s, _name(text))
    for text, s in sorted(first.items(), key=lambda kv: kv[1]):
        fixture = _gta_fixture('m0')[2] if text == F_TEXT else None
        _check(f'wrnn_taco_decode_forced S={S} sentence {s} ({_name(text)})', dict(mel=outs[s][0], attention=outs[s][1]), text, 1, forced=True,
               fixture=fixture)


# ---- two groups per launch ----
def test_free_running_groups_match_the_plain_call_and_the_reference():
    """Two groups of three, F first in one and last in the other: every sentence `array_equal` to `wrnn_taco_decode_batch` on its group
    alone, F of either group within the bars of the fixture."""
    groups = [([F_TEXT, A_TEXT, C_TEXT], (60,) * 3), ([C_TEXT, A_TEXT, F_TEXT], (60,) * 3)]
    outs = _grouped_free(groups, NO_STOP, 1, RICH)
    for g, ((texts, max_steps), out) in enumerate(zip(groups, outs)):
        for s, ((mel, sc, k), (mel1, sc1, k1)) in enumerate(zip(out, _plain_free(texts, max_steps, NO_STOP, 1, RICH))):
            assert k == k1 == 60 and np.array_equal(mel, mel1) and np.array_equal(sc, sc1), (g, s)
        mel, sc, _ = out[texts.index(F_TEXT)]
        _check(f'wrnn_taco_decode_batch_groups group {g} F', dict(mel=_frames(mel), attention=sc), F_TEXT, 1, fixture=_fixture(1))


def test_forced_groups_match_the_plain_call_and_the_reference():
    """The forced form of the same: two groups of three over (m0's mel, the seeded mels), against `wrnn_taco_decode_forced` on each group alone."""
    from wavernn_amd import _lib
    L, w = _lib.lib(), _tts(1, RICH).decoder_weights()
    groups = [[F_TEXT, A_TEXT, C_TEXT], [C_TEXT, A_TEXT, F_TEXT]]

    def call(texts):
        mels = [_forced_mel(t) for t in texts]
        return _forced_call(texts, [m.shape[1] for m in mels], 1, RICH, mels)
    plain = []
    for texts in groups:
        c = call(texts)
        assert L.wrnn_taco_decode_forced(0, ctypes.byref(w), ctypes.byref(c[0])) == _lib.WRNN_OK, L.wrnn_taco_last_error()
        plain.append(_forced_read(c))
    calls = [call(texts) for texts in groups]
    table = (ctypes.POINTER(_lib.TacoForcedCall) * 2)(*[ctypes.pointer(c[0]) for c in calls])
    assert L.wrnn_taco_decode_forced_groups(0, ctypes.byref(w), table, 2) == _lib.WRNN_OK, L.wrnn_taco_last_error()
    for g, (texts, c, ref) in enumerate(zip(groups, calls, plain)):
        got = _forced_read(c)
        for s, ((m, a), (m1, a1)) in enumerate(zip(got, ref)):
            assert np.array_equal(m, m1) and np.array_equal(a, a1), (g, s)
        m, a = got[texts.index(F_TEXT)]
        _check(f'wrnn_taco_decode_forced_groups group {g} F', dict(mel=_frames(m[:30]), attention=a[:30]), F_TEXT, 1, forced=True,
               fixture=_gta_fixture('m0')[2])
