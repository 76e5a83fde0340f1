"""INTEGRATION.md section 1 as a test: the reference's OWN `gen_wavernn.py` flow (`gen_from_file`, gen_wavernn.py:38-65) with the
one-line import swap `from wavernn_amd.model import WaveRNN`.  tests/golden/reference_gen_wavernn.npz holds what that flow produced with the
reference class (scripts/make_golden.py): output file name, waveform, and the next draws of the global generator.  No GPU here, so the
two device entry points of the class are replaced by CPU stand-ins built on the oracle (test infrastructure) -- what is under test is
everything else the reference's script touches: constructor signature, `load()` of a reference state dict, `get_step()`, the `.npy`
checks, `generate()`'s signature / file naming / return value / RNG consumption / train-eval side effects.  The flow is the project's
own `wavernn_amd.gen_wavernn.gen_from_file` (its restatement of the script's `.npy` branch); the result must equal the reference's."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN


class _OracleEngine:
    """CPU stand-in with LoopEngine's face (run / plan / last_*): the oracle's C loop."""

    def __init__(self, sd, mode):
        self.sd, self.mode = sd, mode

    def plan(self, n, T, **kw):
        return dict(kernel='oracle')

    def run(self, mels_up, aux, B, T, stride, noise, hop, out=None, t_range=None, **kw):
        from oracle import c_oracle as C
        assert t_range is None
        mu, au, nz = mels_up.numpy(), aux.numpy(), noise.numpy()
        L = mu.shape[0]
        mels_f = np.zeros((B, T, mu.shape[1]), np.float32)
        aux_f = np.zeros((B, T, au.shape[1]), np.float32)
        for b in range(B):
            p = b * stride + np.arange(T)
            ok = p < L
            mels_f[b, ok] = mu[p[ok]]
            aux_f[b, ok] = au[p[ok] // hop]
        nzo = (np.ascontiguousarray(nz[:, :10 * B].reshape(T, B, 10)), np.ascontiguousarray(nz[:, 10 * B:])) if self.mode == 'MOL' \
            else np.ascontiguousarray(nz.reshape(T, B, -1))
        return torch.from_numpy(C.loop(self.sd, self.mode, mels_f, aux_f, nzo))

    def last_loop_ms(self):
        return 0.0

    def last_loop_kernel(self):
        return 'oracle'


HP = dict(rnn_dims=512, fc_dims=512, bits=9, pad=2, upsample_factors=(5, 5, 11), feat_dims=80, compute_dims=128, res_out_dims=128,
          res_blocks=10, hop_length=275, sample_rate=22050)          # hparams.py:38-50 as gen_wavernn.py:112-123 passes them


@pytest.mark.parametrize('mode', ['RAW', 'MOL'])
def test_reference_gen_wavernn_runs_with_the_import_swap(mode, tmp_path, monkeypatch):
    import wavernn_amd.model as ours
    from wavernn_amd.gen_wavernn import gen_from_file
    from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED
    g = np.load(os.path.join(GOLDEN, 'reference_gen_wavernn.npz'))
    kw = dict(HP, mode=mode)
    assert {k: kw[k] for k in SHIPPED} == SHIPPED
    sd = random_state_dict(17, mode=mode)
    ckpt = tmp_path / 'latest_weights.pyt'
    torch.save(dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, step=torch.tensor([123456])), ckpt)   # the reference's save()
    np.save(tmp_path / 'utt.npy', random_mel(5, 40))
    written = {}

    # ours, with the two device entry points mocked onto the CPU
    monkeypatch.setattr(ours.WaveRNN, '_require_hip_device', staticmethod(lambda device: None))
    monkeypatch.setattr(ours.WaveRNN, '_loop_engine', lambda self: _OracleEngine({k: v.detach().numpy() for k, v in self.state_dict().items()}, self.mode))
    monkeypatch.setattr(ours, 'save_wav', lambda x, path, sr: written.update(path=str(path), x=x.astype(np.float32)))

    class Swapped(ours.WaveRNN):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.pre_algo, self.post_algo = 'torch', 'numpy'

    model = Swapped(**kw)
    model.load(ckpt)                                                                      # gen_wavernn.py:129
    assert model.get_step() == 123456
    os.makedirs(tmp_path / 'ours')
    torch.manual_seed(4242)
    wav, path = gen_from_file(model, tmp_path / 'utt.npy', tmp_path / 'ours', True, 1100, 55)     # the project's gen_wavernn.py:38-65
    assert model.training                                                                 # generate() leaves train mode on (:262)
    after = torch.empty(3).uniform_(0, 1).numpy()                                         # the generator moved exactly as far
    name = os.path.basename(written['path'])
    assert written['path'] == str(path) and np.array_equal(written['x'], np.asarray(wav, np.float32))
    # the reference's script puts the checkpoint's step in thousands into the name; the project's CLI does not
    assert str(g[f'{mode}_name']) == f'__utt__{model.get_step() // 1000}k_steps_gen_batched_target1100_overlap55.wav'
    assert name == '__utt__gen_batched_target1100_overlap55.wav'
    assert np.array_equal(after, g[f'{mode}_after'])
    ref_wav = g[f'{mode}_wav']
    assert written['x'].shape == ref_wav.shape
    if mode == 'RAW':
        assert np.array_equal(written['x'], ref_wav)
    else:
        assert np.abs(written['x'] - ref_wav).max() <= 1e-5
    np.save(tmp_path / 'bad.npy', 2 * random_mel(5, 40))
    with pytest.raises(ValueError, match='range'):                                        # gen_wavernn.py:50-55 guards the input
        gen_from_file(Swapped(**kw), tmp_path / 'bad.npy', tmp_path / 'ours', True, 1100, 55)
    np.save(tmp_path / 'flat.npy', random_mel(5, 40)[0])
    with pytest.raises(ValueError, match='shaped'):
        gen_from_file(Swapped(**kw), tmp_path / 'flat.npy', tmp_path / 'ours', True, 1100, 55)
