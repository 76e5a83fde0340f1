"""One pass of `generate_corpus` around the loop kernel, the new order against the old one: three ragged utterances (24, 53 and 60 frames; MoL,
finish='own', noise from the device generator under a fixed seed).  The pre-loop stages batched into one launch each (`model.pre_batched`,
wrnn_pre_upsample_many) against utterance by utterance (`pre_streams = 1`) and side streams (8); the post-loop tables on the device before the loop is queued
(`model.post_tables_early`) against behind it; the one-launch slab preparation against the three calls (`model.slab_prep_split`): the same waveforms,
bit for bit, every way."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, TARGET, OVERLAP, HOP, SEED = (24, 53, 60), 550, 55, 275, 1234


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def setup(gpu):
    """The model, the mels and the waveforms of the default settings: computed once."""
    from wavernn_amd.model import WaveRNN
    from wavernn_amd.synthetic import random_mel, random_state_dict, SHIPPED
    model = WaveRNN(**SHIPPED, mode='MOL')
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(61, mode='MOL').items()}, strict=True)
    model = model.to(gpu).eval()
    mels = [torch.from_numpy(random_mel(1900 + k, n)).unsqueeze(0).to(gpu) for k, n in enumerate(FRAMES)]
    assert (model.pre_batched, model.post_tables_early, model.slab_prep_split) == (True, True, False)
    return model, mels, _run(model, mels)


def _run(model, mels, **settings):
    from wavernn_amd.batch import generate_corpus
    was = {k: getattr(model, k) for k in settings}
    for k, v in settings.items():
        setattr(model, k, v)
    try:
        torch.manual_seed(SEED)
        outs = generate_corpus(model, mels, TARGET, OVERLAP, True, None, noise_source='device', finish='own')
    finally:
        for k, v in was.items():
            setattr(model, k, v)
    return [np.array(o, copy=True) for o in outs]


def _same(a, b):
    assert len(a) == len(b) == len(FRAMES)
    for u, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == np.float64 and x.shape == y.shape == ((FRAMES[u] - 1) * HOP,)
        assert np.array_equal(x, y), f'utterance {u}: {int((x != y).sum())} samples differ'


def test_default_pass_is_sane(setup):
    model, mels, base = setup
    for w in base:
        assert np.isfinite(w).all() and np.abs(w).max() <= 1.0 and w.std() > 1e-3
    assert w[-1] == 0.0                                     # (the tail fade ends at 0)
    _same(base, _run(model, mels))                          # the same seed, the same audio: what the comparisons below rest on


@pytest.mark.parametrize('streams', [1, 8])
def test_batched_pre_loop_against_per_utterance(setup, streams):
    model, mels, base = setup
    _same(base, _run(model, mels, pre_batched=False, pre_streams=streams))


def test_tables_early_against_behind_the_loop(setup):
    model, mels, base = setup
    _same(base, _run(model, mels, post_tables_early=False))


def test_slab_prep_fused_against_three_calls(setup):
    model, mels, base = setup
    _same(base, _run(model, mels, slab_prep_split=True))


def test_everything_as_before(setup):
    model, mels, base = setup
    _same(base, _run(model, mels, pre_batched=False, pre_streams=8, post_tables_early=False, slab_prep_split=True))
