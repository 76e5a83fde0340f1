"""Generate tests/golden/score_loss_cases.npz and tests/golden/score_forward_3utt.npz by RUNNING THE REFERENCE ITSELF (CPU).

The fixtures of the scoring path (wavernn_amd/score.py, csrc/wrnn_nll.hip): what the reference's own loss functions and its own teacher-forced
`WaveRNN.forward` return.  Like scripts/make_golden.py this runs only where the reference checkout is mounted (WRNN_REFERENCE, read-only), with
the same shims -- a stub `librosa`, `np.cumproduct`, `hparams` configured --, writes nothing into the reference tree, and the .npz files are
committed.

    python scripts/make_golden_score.py
"""
import os, sys, types
import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF = os.environ.get('WRNN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
lib = types.ModuleType('librosa'); lib.output = types.SimpleNamespace(write_wav=lambda *a, **k: None)
sys.modules['librosa'] = lib
if not hasattr(np, 'cumproduct'):
    np.cumproduct = np.cumprod
import torch
import torch.nn.functional as F
from utils import hparams as hp
hp.configure(os.path.join(REF, 'hparams.py'))
from models.fatchord_version import WaveRNN          # the reference implementation
from utils.distribution import discretized_mix_logistic_loss
from utils.dsp import float_2_label, label_2_float, encode_mu_law

from wavernn_amd.synthetic import random_state_dict, random_mel, score_loss_inputs, SHIPPED

OUT = os.path.join(REPO, 'tests', 'golden')
HOP = SHIPPED['hop_length']


def ref_mol(logits, y):
    """logits (n, T, 30), y (n, T) -> the reference's per-element loss (n, T)"""
    return discretized_mix_logistic_loss(logits, y.unsqueeze(-1), reduce=False)[..., 0]


def ref_raw(logits, labels):
    """logits (n, T, C), labels (n, T) int64 -> per-element F.cross_entropy in the shapes train_wavernn.py:115-123 gives it"""
    return F.cross_entropy(logits.transpose(1, 2).unsqueeze(-1), labels.unsqueeze(-1), reduction='none')[..., 0]


def loss_cases():
    # the inputs are seeded (wavernn_amd.synthetic.score_loss_inputs: the tests rebuild them); stored: targets, labels, every 97th input value
    # and the reference's results
    lg, lab = score_loss_inputs('mol')
    logits = torch.from_numpy(lg).transpose(0, 1).contiguous()                 # (n, T, 30), as the reference's loss takes it
    y = label_2_float(torch.from_numpy(lab).float(), 16)
    assert y.dtype == torch.float32 and float(y.min()) == -1.0 and float(y.max()) == 1.0
    assert abs(float(y[lab == 16].mean()) + 0.9995) < 2e-5
    ref32, ref64 = ref_mol(logits, y), ref_mol(logits.double(), y.double())
    # branch shares of the set (float64 restatement of the three conditions)
    yy, ls = y.double().unsqueeze(-1), logits[..., 20:].double()
    inv = torch.exp(-ls)
    cy = yy - logits[..., 10:20].double()
    delta = torch.sigmoid(inv * (cy + 1 / 65535)) - torch.sigmoid(inv * (cy - 1 / 65535))
    share_lo, share_hi, share_delta = float((y < -0.999).float().mean()), float((y > 0.999).float().mean()), float((delta > 1e-5).float().mean())
    print(f'MOL loss cases: y < -0.999 {share_lo:.3f}, y > 0.999 {share_hi:.3f}, cdf_delta > 1e-5 {share_delta:.3f}; '
          f'max |ref32 - ref64| = {float((ref32.double() - ref64).abs().max()):.3e}')
    assert share_lo >= 0.02 and share_hi >= 0.02 and 0.2 <= share_delta <= 0.9
    out = dict(seed=np.int32(4100), mol_logits_strided=lg.reshape(-1)[::97], mol_target=y.numpy(), mol_labels=lab.astype(np.uint16),
               mol_ref32=ref32.numpy(), mol_ref64=ref64.numpy())
    for C in (512, 256):
        lg, lab = score_loss_inputs(f'raw{C}')
        logits, lab = torch.from_numpy(lg).transpose(0, 1).contiguous(), torch.from_numpy(lab)
        ref32, ref64 = ref_raw(logits, lab), ref_raw(logits.double(), lab)
        print(f'RAW {C} loss cases: max |ref32 - ref64| = {float((ref32.double() - ref64).abs().max()):.3e}')
        out.update({f'raw{C}_logits_strided': lg.reshape(-1)[::97], f'raw{C}_target': label_2_float(lab.float(), int(np.log2(C))).numpy(),
                    f'raw{C}_labels': lab.numpy().astype(np.int16), f'raw{C}_ref32': ref32.numpy(), f'raw{C}_ref64': ref64.numpy()})
    path = os.path.join(OUT, 'score_loss_cases.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


FRAMES = (9, 17, 24)
WSEED = dict(MOL=12, RAW=11)


def waveform(u, n):
    """a ramped sine plus noise, clipped (some samples sit at exactly +-1)"""
    rs = np.random.RandomState(300 + u)
    t = np.arange(n)
    w = np.linspace(0.1, 1.15, n) * np.sin(2 * np.pi * (180.0 + 40 * u) * t / SHIPPED['sample_rate']) + 0.03 * rs.standard_normal(n)
    return np.clip(w, -1, 1).astype(np.float32)


def forward_cases():
    out = dict(frames=np.array(FRAMES, np.int32), mel_seeds=np.array([103 + u for u in range(len(FRAMES))], np.int32),
               wseed_mol=np.int32(WSEED['MOL']), wseed_raw=np.int32(WSEED['RAW']), logits_stride=np.int32(97))
    wavs = [waveform(u, n * HOP) for u, n in enumerate(FRAMES)]
    for u, w in enumerate(wavs):
        out[f'wav{u}'] = w
        out[f'labels16_{u}'] = float_2_label(w, bits=16).astype(np.int64).astype(np.uint16)                 # preprocess.py:45, :47
        out[f'labels9_{u}'] = float_2_label(w, bits=9).astype(np.int64).astype(np.int16)                    # :43 with hp.mu_law off
        out[f'labels9mu_{u}'] = encode_mu_law(w, mu=2 ** 9).astype(np.int64).astype(np.int16)               # :43
    for mode in ('MOL', 'RAW'):
        sd = random_state_dict(WSEED[mode], mode=mode)
        model = WaveRNN(**SHIPPED, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        model.eval()
        bits = 16 if mode == 'MOL' else 9
        sens = 0.0
        rs = np.random.RandomState(4200)
        for u, n in enumerate(FRAMES):
            lab = torch.from_numpy(out[f'labels16_{u}' if mode == 'MOL' else f'labels9mu_{u}'].astype(np.int64))
            y = label_2_float(lab.float(), bits)                                                            # utils/dataset.py:88-91
            x = torch.cat([torch.zeros(1), y[:-1]])
            mel = torch.from_numpy(random_mel(103 + u, n)).unsqueeze(0)
            with torch.no_grad():
                m = model.pad_tensor(mel.transpose(1, 2), pad=model.pad, side='both').transpose(1, 2)       # as generate() pads it
                logits = model(x.unsqueeze(0), m)
                assert logits.shape == (1, n * HOP, model.n_classes)
                loss = (lambda lg: ref_mol(lg, y.unsqueeze(0))[0]) if mode == 'MOL' else (lambda lg: ref_raw(lg, lab.unsqueeze(0))[0])
                nll = loss(logits)
                for _ in range(4):
                    sign = torch.from_numpy(np.where(rs.random_sample(tuple(logits.shape)) < 0.5, -1.0, 1.0).astype(np.float32))
                    sens = max(sens, float((loss(logits + 1e-4 * sign) - nll).abs().max()))
            k = mode.lower()
            out[f'{k}_target{u}'] = y.numpy()
            out[f'{k}_nll{u}'] = nll.numpy()
            out[f'{k}_logits{u}'] = logits[0, ::97].numpy()
            print(f'{mode} utterance {u}: {n * HOP} steps, mean nll {float(nll.double().mean()):.6f}, sensitivity so far {sens:.3e}')
        out[f'{mode.lower()}_nll_mean'] = np.array([np.float64(out[f'{mode.lower()}_nll{u}'].astype(np.float64).mean()) for u in range(len(FRAMES))])
        out[f'{mode.lower()}_nll_sensitivity'] = np.float64(sens)
    path = os.path.join(OUT, 'score_forward_3utt.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    loss_cases()
    forward_cases()
