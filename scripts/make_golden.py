"""Generate tests/golden/*.npz by RUNNING THE REFERENCE ITSELF (CPU) in the build container.

The reference (fatchord/WaveRNN, mounted read-only at /root/reference) has no tests or golden vectors,
so the fixtures pinning `oracle/` are outputs of the reference's own `WaveRNN.generate()` under a
fixed seed.  /root/reference does not exist on the GPU box: this script runs only here, the .npz
fixtures are committed.  Shims: stub `librosa`, alias `np.cumproduct`,
configure `hparams`.  Nothing is written into the reference tree.

    python scripts/make_golden.py
    python scripts/make_golden.py planner_table     # tests/golden/planner_table.npz only: the built library's launch planner, no reference needed
"""
import os, sys, types
import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF = os.environ.get('WRNN_REFERENCE', '/root/reference')


# ---- tests/golden/planner_table.npz: the launch planner, recorded through wrnn_debug_plan.  Needs the built library only (neither a GPU
# nor the reference): `python scripts/make_golden.py planner_table` leaves before the reference is imported. ------------------------------
PLAN_TRAITS = ('n_cus', 'mode', 'C', 'generic', 'gH', 'gF', 'gM', 'gA', 'sp_nbp', 'sp_max_blocks', 'sp_fc')
PLAN_CALL = ('algo', 'n_segments', 'T', 'n_frames', 'depth', 'clusters', 'slab_steps', 't_begin', 't_end')
PLAN_OUT = ('rc', 'kernel', 'units_per_wg', 'clusters', 'depth', 'rounds', 'slab_steps', 'workspace_bytes', 'error')
PLAN_CUS = (32, 64, 128, 192, 255, 256, 304)
PLAN_PACKS = dict(                    # mode: 0 RAW, 1 MOL
    dense_mol=dict(mode=1, C=30, sp_max_blocks=512),
    dense_raw512=dict(mode=0, C=512, sp_max_blocks=512),
    raw256=dict(mode=0, C=256, sp_max_blocks=512),
    sparse_mol_48=dict(mode=1, C=30, sp_nbp=48, sp_max_blocks=40),
    sparse_mol_64=dict(mode=1, C=30, sp_nbp=64, sp_max_blocks=60),
    sparse_mol_64_fc=dict(mode=1, C=30, sp_nbp=64, sp_max_blocks=60, sp_fc=1),
    sparse_raw512=dict(mode=0, C=512, sp_nbp=64, sp_max_blocks=60, sp_fc=1),
    generic=dict(mode=1, C=30, generic=1, gH=256, gF=256, gM=80, gA=32, sp_max_blocks=256))
PLAN_ALGOS = (0, 1, 2, 5, 6, 7, 8, 3, 4, 9)         # auto, stream, loop, sparse, duo, chain, octo; 3, 4, 9: unknown
PLAN_SEGMENTS = (1, 16, 17, 64, 65, 128, 129, 256, 257, 300, 512, 513, 942, 4096, 43690, 43691)     # the last two: either side of the 2 GB aux-table refusal


def planner_cases():
    """The rows of the table, as dicts of PLAN_TRAITS + PLAN_CALL: the full cross of device size x pack x algo x segment count at default
    options, and the option axes (depth x clusters; T x slab_steps x n_frames; step ranges) on fewer devices and packs."""
    from itertools import product
    rows = []

    def add(cus, pack, algo, n, T=12100, n_frames=700, depth=0, clusters=0, slab_steps=0, t_range=(0, 0)):
        rows.append(dict(dict.fromkeys(PLAN_TRAITS, 0), **PLAN_PACKS[pack], n_cus=cus, algo=algo, n_segments=n, T=T, n_frames=n_frames, depth=depth,
                         clusters=clusters, slab_steps=slab_steps, t_begin=t_range[0], t_end=t_range[1]))
    for cus, pack, algo, n in product(PLAN_CUS, PLAN_PACKS, PLAN_ALGOS, PLAN_SEGMENTS):
        add(cus, pack, algo, n)
    for cus, pack, algo, n, depth, clusters in product((128, 256, 304), ('dense_mol', 'dense_raw512', 'sparse_mol_64_fc'), (0, 2, 5, 6, 7, 8),
                                                       (1, 65, 300, 942), (0, 1, 2, 3, 4, 8, 9), (0, 1, 2, 3, 4)):
        add(cus, pack, algo, n, depth=depth, clusters=clusters)
    for cus, pack, algo, n, T, slab, nf in product((64, 256), ('dense_mol', 'dense_raw512', 'raw256', 'sparse_mol_64', 'generic'), PLAN_ALGOS[:7],
                                                   (1, 129, 942), (1, 100, 12100), (0, 97, 5000), (1, 700)):
        add(cus, pack, algo, n, T=T, n_frames=nf, slab_steps=slab)
    for cus, pack, algo, n, rng in product((32, 256), ('dense_mol', 'raw256', 'sparse_mol_48', 'generic'), (0, 1, 2, 5, 6, 7, 9), (1, 300),
                                           ((0, 0), (10, 60), (0, 100), (60, 10), (-1, 50), (0, 101), (100, 100))):
        add(cus, pack, algo, n, T=100, t_range=rng)
    return rows


def plan_one(L, row):
    """One row through wrnn_debug_plan -> (rc, kernel name, units_per_wg, clusters, depth, rounds, slab_steps, workspace bytes, error text)."""
    import ctypes
    from wavernn_amd import _lib
    t = _lib.PlanTraits(**{k: row[k] for k in PLAN_TRAITS})
    o = _lib.Options(algo=row['algo'], depth=row['depth'], clusters=row['clusters'], slab_steps=row['slab_steps'], t_begin=row['t_begin'],
                     t_end=row['t_end'])
    i, ws = _lib.RunInfo(), ctypes.c_size_t(0)
    rc = L.wrnn_debug_plan(ctypes.byref(t), row['n_segments'], row['T'], row['n_frames'], ctypes.byref(o), ctypes.byref(i), ctypes.byref(ws))
    if rc != 0:
        return (rc, None, 0, 0, 0, 0, 0, 0, L.wrnn_last_error().decode())
    return (rc, i.kernel.decode(), i.units_per_wg, i.clusters, i.depth, i.rounds, i.slab_steps, ws.value, None)


def planner_table():
    import io, zipfile
    from wavernn_amd import _lib
    L = _lib.lib()
    rows = planner_cases()
    kernels, errors, outs = [], [], []
    for r in rows:
        res = list(plan_one(L, r))
        for col, names in ((1, kernels), (8, errors)):      # names -> indices into de-duplicated lists (-1: none)
            if res[col] is None:
                res[col] = -1
            else:
                if res[col] not in names:
                    names.append(res[col])
                res[col] = names.index(res[col])
        outs.append(res)
    arrays = dict(traits=np.array([[r[k] for k in PLAN_TRAITS] for r in rows], np.int32), trait_names=np.array(PLAN_TRAITS),
                  call=np.array([[r[k] for k in PLAN_CALL] for r in rows], np.int32), call_names=np.array(PLAN_CALL),
                  out=np.array(outs, np.int64), out_names=np.array(PLAN_OUT), kernels=np.array(kernels), errors=np.array(errors))
    # an .npz with fixed member dates: the same table gives the same file, byte for byte
    path = os.path.join(REPO, 'tests', 'golden', 'planner_table.npz')
    with zipfile.ZipFile(path, 'w') as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    print('planner table:', len(rows), 'rows,', len(kernels), 'kernels,', len(errors), 'error texts,', os.path.getsize(path), 'bytes')


if __name__ == '__main__' and sys.argv[1:] == ['planner_table']:
    planner_table()
    sys.exit(0)

sys.path.insert(0, REF)
lib = types.ModuleType('librosa'); lib.output = types.SimpleNamespace(write_wav=lambda *a, **k: None)
sys.modules['librosa'] = lib
if not hasattr(np, 'cumproduct'):
    np.cumproduct = np.cumprod
import torch
from utils import hparams as hp
hp.configure(os.path.join(REF, 'hparams.py'))
from models.fatchord_version import WaveRNN          # the reference implementation
WaveRNN.gen_display = lambda self, *a, **k: None

from wavernn_amd.synthetic import random_state_dict, random_mel, SHIPPED

OUT = os.path.join(REPO, 'tests', 'golden')

CASES = [
    # name, mode, weight seed, mel seed, frames, batched, target, overlap, mu_law, sample seed
    dict(name='raw_unbatched_24f', mode='RAW', wseed=11, mseed=101, frames=24, batched=False, target=11000, overlap=550, mu_law=True, seed=77),
    dict(name='raw_batched_60f', mode='RAW', wseed=11, mseed=102, frames=60, batched=True, target=1100, overlap=55, mu_law=True, seed=78),
    dict(name='mol_unbatched_24f', mode='MOL', wseed=12, mseed=103, frames=24, batched=False, target=11000, overlap=550, mu_law=True, seed=79),
    dict(name='mol_batched_100f', mode='MOL', wseed=12, mseed=104, frames=100, batched=True, target=1100, overlap=55, mu_law=True, seed=80),
    dict(name='mol_batched_ragged_53f', mode='MOL', wseed=13, mseed=105, frames=53, batched=True, target=2000, overlap=100, mu_law=False, seed=81),
    # BASELINE config 2 at its stated inputs: weight seed 0, mel seed 1234, N=481 -> B=12, T=12100, sample seed 77
    dict(name='mol_batched_481f', mode='MOL', wseed=0, mseed=1234, frames=481, batched=True, target=11000, overlap=550, mu_law=True, seed=77),
    dict(name='raw_batched_481f', mode='RAW', wseed=0, mseed=1234, frames=481, batched=True, target=11000, overlap=550, mu_law=True, seed=77),
    # BASELINE config 3, vocoder side (gen_tacotron.py:139-166): the mel comes from the reference's own Tacotron.generate
    # (seeded random init, steps=800 -> (80,800)), rescaled (m+4)/8 and clipped (:144-145); L = 220,000 = 19*11,550 + 550
    # exactly -> B = 19 with NO padded fold.  The mel is stored in the fixture (Tacotron is upstream of the path).
    dict(name='mol_tacotron_800f', mode='MOL', wseed=0, mseed=None, frames=800, batched=True, target=11000, overlap=550, mu_law=True, seed=77,
         tts_seed=3),
    # Round 6: the two utterances of the 64-utterance RAW flip-rate measurement (scripts/gpu_raw_flips.py: weight seed 0, mel seed 1234 + u,
    # sample seed 77 + u, 641 frames -> 16 segments x 12,100 steps) in which a kernel's class indices parted ways with the C ORACLE -- u = 34
    # (segment 2, step 7,399: the oracle itself is the odd one out there) and u = 46 (segment 14, step 3,015).  `compact`: only the
    # reference's class indices are stored ([B, T] uint16; the float sample is 2 idx / 511 - 1).
    dict(name='raw_flip_u34', mode='RAW', wseed=0, mseed=1268, frames=641, batched=True, target=11000, overlap=550, mu_law=True, seed=111, compact=True),
    dict(name='raw_flip_u46', mode='RAW', wseed=0, mseed=1280, frames=641, batched=True, target=11000, overlap=550, mu_law=True, seed=123, compact=True),
]


def tacotron_mel(c):
    """gen_tacotron.py:97-145 with a seeded random-init Tacotron: first line of sentences.txt -> text_to_sequence ->
    Tacotron.generate(x, steps=frames) -> (m + 4) / 8, clip to [0, 1].  Stubs: unidecode, inflect."""
    import time
    un = types.ModuleType('unidecode'); un.unidecode = lambda s: s
    sys.modules.setdefault('unidecode', un)
    inf = types.ModuleType('inflect'); inf.engine = lambda: types.SimpleNamespace(number_to_words=lambda *a, **k: 'number')
    sys.modules.setdefault('inflect', inf)
    from models.tacotron import Tacotron
    from utils.text.symbols import symbols
    from utils.text import text_to_sequence
    torch.manual_seed(c['tts_seed'])
    tts = Tacotron(embed_dims=hp.tts_embed_dims, num_chars=len(symbols), encoder_dims=hp.tts_encoder_dims,
                   decoder_dims=hp.tts_decoder_dims, n_mels=hp.num_mels, fft_bins=hp.num_mels, postnet_dims=hp.tts_postnet_dims,
                   encoder_K=hp.tts_encoder_K, lstm_dims=hp.tts_lstm_dims, postnet_K=hp.tts_postnet_K,
                   num_highways=hp.tts_num_highways, dropout=hp.tts_dropout, stop_threshold=hp.tts_stop_threshold)
    with open(os.path.join(REF, 'sentences.txt')) as f:
        x = text_to_sequence(f.readline().strip(), hp.tts_cleaner_names)
    t0 = time.perf_counter()
    with torch.no_grad():
        _, m, _ = tts.generate(x, steps=c['frames'])
    print(f'reference Tacotron.generate: {len(x)} symbols -> mel {m.shape} in {time.perf_counter() - t0:.1f} s (CPU, {torch.get_num_threads()} threads)')
    m = (m + 4) / 8
    np.clip(m, 0, 1, out=m)
    assert m.shape == (80, c['frames']), m.shape
    return np.ascontiguousarray(m, dtype=np.float32)


def run_case(c):
    sd_np = random_state_dict(c['wseed'], mode=c['mode'])
    model = WaveRNN(**SHIPPED, mode=c['mode'])
    missing = model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd_np.items()}, strict=True)
    mel = tacotron_mel(c) if c['mseed'] is None else random_mel(c['mseed'], c['frames'])
    cap = {}
    real_stack = torch.stack

    def stack(tensors, *a, **k):
        r = real_stack(tensors, *a, **k)
        cap['raw'] = r
        return r

    # conditioning tensors the reference feeds the loop (for the upsample/fold oracle checks)
    real_up = model.upsample.forward

    def up(m):
        a, b = real_up(m)
        cap['mels_up'], cap['aux_up'] = a.detach().clone(), b.detach().clone()
        return a, b
    model.upsample.forward = up
    torch.stack = stack
    try:
        torch.manual_seed(c['seed'])
        import time
        t0 = time.perf_counter()
        out = model.generate(torch.tensor(mel).unsqueeze(0), '/tmp/_golden.wav', c['batched'], c['target'],
                             c['overlap'], c['mu_law'])
        c = dict(c, ref_cpu_seconds=round(time.perf_counter() - t0, 2), ref_cpu_threads=torch.get_num_threads())
    finally:
        torch.stack = real_stack
    raw = cap['raw'].transpose(0, 1).contiguous().numpy()       # (B,T) float32, pre-decode (:243)
    if c.get('compact'):
        idx = np.rint((raw.astype(np.float64) + 1.0) * 511.0 / 2.0).astype(np.uint16)
        assert np.array_equal(idx.astype(np.float32) * np.float32(2) / np.float32(511) - np.float32(1), raw)
        np.savez_compressed(os.path.join(OUT, c['name'] + '.npz'), config=np.array(repr(c)), cls=idx, n_classes=np.int64(512))
        print(c['name'], 'class indices', idx.shape, 'min', idx.min(), 'max', idx.max())
        return
    mels_up = cap['mels_up'][0].numpy()
    aux_up = cap['aux_up'][0].numpy()
    # keep fixtures small: conditioning is stored strided (every 97th upsampled sample) + full aux frames
    extra = {'mel': mel.astype(np.float32)} if c['mseed'] is None else {}
    np.savez_compressed(os.path.join(OUT, c['name'] + '.npz'), **extra,
                        config=np.array(repr(c)), out=out.astype(np.float64), raw=raw.astype(np.float32),
                        mels_up_strided=mels_up[::97].astype(np.float32), aux_up_strided=aux_up[::97].astype(np.float32),
                        L=np.int64(mels_up.shape[0]))
    print(c['name'], 'raw', raw.shape, 'out', out.shape, 'absmax', np.abs(out).max())


def rng_kats():
    """Known-answer vectors of torch's CPU generator for the RNG oracle."""
    torch.manual_seed(5)
    u = torch.empty(16).uniform_(0, 1).numpy()
    torch.manual_seed(5)
    u2 = torch.empty(16).uniform_(1e-5, 1 - 1e-5).numpy()
    torch.manual_seed(5)
    e = torch.empty(16).exponential_(1).numpy()
    torch.manual_seed(9)
    _ = torch.nn.GRUCell(512, 512); _ = torch.nn.GRUCell(544, 512)
    after = torch.empty(8).uniform_(1e-5, 1 - 1e-5).numpy()
    torch.manual_seed(21)
    mix = [torch.empty(1, 3, 10).uniform_(1e-5, 1 - 1e-5).numpy().ravel(), torch.empty(1, 3).uniform_(1e-5, 1 - 1e-5).numpy().ravel(),
           torch.empty(1, 3, 10).uniform_(1e-5, 1 - 1e-5).numpy().ravel(), torch.empty(1, 3).uniform_(1e-5, 1 - 1e-5).numpy().ravel()]
    torch.manual_seed(22)
    ex = torch.empty(3, 512).exponential_(1).numpy()
    np.savez_compressed(os.path.join(OUT, 'rng_kats.npz'), uniform01_seed5=u, uniform_mol_seed5=u2, exp_seed5=e,
                        after_grucell_ctors_seed9=after, mol_two_steps_seed21=np.concatenate(mix), exp_3x512_seed22=ex)
    print('rng kats written')


def tacotron_shapes():
    """Key / shape / dtype table of the reference Tacotron's state dict (hparams.py tts_*): lets the GPU box build a random-init
    Tacotron state dict of the right architecture without the reference (tests/test_gpu_config3.py)."""
    import json
    c = dict(mseed=None, tts_seed=3, frames=1)
    un = types.ModuleType('unidecode'); un.unidecode = lambda s: s
    sys.modules.setdefault('unidecode', un)
    inf = types.ModuleType('inflect'); inf.engine = lambda: types.SimpleNamespace(number_to_words=lambda *a, **k: 'number')
    sys.modules.setdefault('inflect', inf)
    from models.tacotron import Tacotron
    from utils.text.symbols import symbols
    tts = Tacotron(embed_dims=hp.tts_embed_dims, num_chars=len(symbols), encoder_dims=hp.tts_encoder_dims,
                   decoder_dims=hp.tts_decoder_dims, n_mels=hp.num_mels, fft_bins=hp.num_mels, postnet_dims=hp.tts_postnet_dims,
                   encoder_K=hp.tts_encoder_K, lstm_dims=hp.tts_lstm_dims, postnet_K=hp.tts_postnet_K,
                   num_highways=hp.tts_num_highways, dropout=hp.tts_dropout, stop_threshold=hp.tts_stop_threshold)
    table = [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in tts.state_dict().items()]
    json.dump(table, open(os.path.join(OUT, 'tacotron_shapes.json'), 'w'))
    print('tacotron shapes written:', len(table), 'tensors')


def tacotron_decoder_golden(steps=200, wseed=3):
    """What the reference's own `Tacotron.generate` (models/tacotron.py:370-430) returns for the weights the GPU tests use:
    `random_tacotron_state_dict(3, shapes)` loaded into the REFERENCE class, first line of sentences.txt, `steps` decoder steps.
    tests/test_gpu_config3.py compares both decoder kernels and the CBHG GRU kernel's post-net to these arrays on the GPU box
    (SURVEY.md section 8 row f3); tests/test_oracle_golden.py compares the CPU mirror to them here."""
    import json
    un = types.ModuleType('unidecode'); un.unidecode = lambda s: s
    sys.modules.setdefault('unidecode', un)
    inf = types.ModuleType('inflect'); inf.engine = lambda: types.SimpleNamespace(number_to_words=lambda *a, **k: 'number')
    sys.modules.setdefault('inflect', inf)
    from models.tacotron import Tacotron
    from utils.text.symbols import symbols
    from utils.text import text_to_sequence
    from wavernn_amd.synthetic import random_tacotron_state_dict
    tts = Tacotron(embed_dims=hp.tts_embed_dims, num_chars=len(symbols), encoder_dims=hp.tts_encoder_dims,
                   decoder_dims=hp.tts_decoder_dims, n_mels=hp.num_mels, fft_bins=hp.num_mels, postnet_dims=hp.tts_postnet_dims,
                   encoder_K=hp.tts_encoder_K, lstm_dims=hp.tts_lstm_dims, postnet_K=hp.tts_postnet_K,
                   num_highways=hp.tts_num_highways, dropout=hp.tts_dropout, stop_threshold=hp.tts_stop_threshold)
    shapes = json.load(open(os.path.join(OUT, 'tacotron_shapes.json')))
    sd = {k: torch.as_tensor(np.array(v)) for k, v in random_tacotron_state_dict(wseed, shapes).items()}
    tts.load_state_dict(sd, strict=True)
    with open(os.path.join(REF, 'sentences.txt')) as f:
        ids = text_to_sequence(f.readline().strip(), hp.tts_cleaner_names)
    with torch.no_grad():
        mel, lin, attn = tts.generate(ids, steps=steps)
    mel, lin, attn = np.asarray(mel, np.float32), np.asarray(lin, np.float32), np.asarray(attn, np.float32)
    assert mel.shape == (80, steps) and lin.shape == (80, steps) and attn.shape == (steps, len(ids)), (mel.shape, lin.shape, attn.shape)
    np.savez_compressed(os.path.join(OUT, f'tacotron_decoder_{steps}f.npz'), mel=mel, linear=lin, attention=attn, ids=np.array(ids, np.int32),
                        config=np.array(repr(dict(wseed=wseed, steps=steps, source='reference models/tacotron.py Tacotron.generate, CPU'))))
    print('tacotron decoder golden:', mel.shape, lin.shape, attn.shape, 'mel absmax', float(np.abs(mel).max()))


def _text_stubs():
    un = types.ModuleType('unidecode'); un.unidecode = lambda s: s
    sys.modules.setdefault('unidecode', un)
    inf = types.ModuleType('inflect'); inf.engine = lambda: types.SimpleNamespace(number_to_words=lambda *a, **k: 'number')
    sys.modules.setdefault('inflect', inf)


def _reference_tacotron():
    _text_stubs()
    from models.tacotron import Tacotron
    from utils.text.symbols import symbols
    return Tacotron(embed_dims=hp.tts_embed_dims, num_chars=len(symbols), encoder_dims=hp.tts_encoder_dims,
                    decoder_dims=hp.tts_decoder_dims, n_mels=hp.num_mels, fft_bins=hp.num_mels, postnet_dims=hp.tts_postnet_dims,
                    encoder_K=hp.tts_encoder_K, lstm_dims=hp.tts_lstm_dims, postnet_K=hp.tts_postnet_K,
                    num_highways=hp.tts_num_highways, dropout=hp.tts_dropout, stop_threshold=hp.tts_stop_threshold)


def tacotron_mirror_golden(wseed=5):
    """tests/golden/tacotron_mirror.npz (tests/test_tacotron_mirror.py): the reference's own `Tacotron.generate` for
    `rich_tacotron_state_dict(5)` (tests/helpers.py: random matrices, biases and batch norms) on the first line of sentences.txt --
    r = 1 for 60 and 800 steps, r = 3 for 30 steps --, and the two outputs of the torch-initialised `torch.manual_seed(3)` Tacotron
    whose post-net output became the mel of mol_tacotron_800f.npz (`_, m, _ = tts.generate(x)`, gen_tacotron.py:142)."""
    import json
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from helpers import rich_tacotron_state_dict
    _text_stubs()
    from utils.text import text_to_sequence
    with open(os.path.join(REF, 'sentences.txt')) as f:
        line = f.readline().strip()
    ids = text_to_sequence(line, hp.tts_cleaner_names)
    shapes = json.load(open(os.path.join(OUT, 'tacotron_shapes.json')))
    tts = _reference_tacotron()
    tts.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in rich_tacotron_state_dict(wseed, shapes).items()}, strict=True)
    out = dict(line=np.array(line), ids=np.array(ids, np.int32), config=np.array(repr(dict(wseed=wseed, fixture_tts_seed=3))))
    with torch.no_grad():
        for tag, r, steps in (('r1_60', 1, 60), ('r1_800', 1, 800), ('r3_30', 3, 30)):
            tts.r = r
            mel, lin, attn = tts.generate(ids, steps=steps)
            out.update({f'mel_{tag}': np.asarray(mel, np.float32), f'linear_{tag}': np.asarray(lin, np.float32),
                        f'attention_{tag}': np.asarray(attn, np.float32)})
        torch.manual_seed(3)
        tts = _reference_tacotron()
        mel, lin, _ = tts.generate(ids, steps=800)
    out.update(fixture_mel=np.asarray(mel, np.float32), fixture_linear=np.asarray(lin, np.float32))
    np.savez_compressed(os.path.join(OUT, 'tacotron_mirror.npz'), **out)
    print('tacotron mirror golden:', {k: v.shape for k, v in out.items()})


def reference_script_golden():
    """tests/golden/reference_gen_wavernn.npz (tests/test_reference_scripts.py): what the reference's own `gen_wavernn.py` flow
    (`gen_from_file`, gen_wavernn.py:38-65) produced with the reference class: output file name, waveform handed to the writer and the
    next three draws of the global generator -- for a checkpoint of `random_state_dict(17)` at step 123456, `random_mel(5, 40)` saved
    as utt.npy, `torch.manual_seed(4242)`, batched, target 1100, overlap 55."""
    import tempfile
    _text_stubs()
    written = {}
    lib.output.write_wav = lambda path, x, sr: written.update(path=str(path), x=np.asarray(x))
    out = {}
    for mode in ('RAW', 'MOL'):
        kw = dict(rnn_dims=hp.voc_rnn_dims, fc_dims=hp.voc_fc_dims, bits=hp.bits, pad=hp.voc_pad, upsample_factors=hp.voc_upsample_factors,
                  feat_dims=hp.num_mels, compute_dims=hp.voc_compute_dims, res_out_dims=hp.voc_res_out_dims, res_blocks=hp.voc_res_blocks,
                  hop_length=hp.hop_length, sample_rate=hp.sample_rate, mode=mode)
        with tempfile.TemporaryDirectory() as td:
            ckpt = os.path.join(td, 'latest_weights.pyt')
            m = WaveRNN(**kw)
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in random_state_dict(17, mode=mode).items()})
            m.step += 123456
            m.save(ckpt)
            np.save(os.path.join(td, 'utt.npy'), random_mel(5, 40))
            sys.modules.pop('gen_wavernn', None)
            import gen_wavernn as G
            model = G.WaveRNN(**kw)
            model.load(ckpt)
            os.makedirs(os.path.join(td, 'out'))
            torch.manual_seed(4242)
            G.gen_from_file(model, __import__('pathlib').Path(td) / 'utt.npy', __import__('pathlib').Path(td) / 'out', True, 1100, 55)
            assert model.training
            after = torch.empty(3).uniform_(0, 1).numpy()
        out[f'{mode}_name'] = np.array(os.path.basename(written['path']))
        out[f'{mode}_wav'] = written['x']
        out[f'{mode}_after'] = after
    np.savez_compressed(os.path.join(OUT, 'reference_gen_wavernn.npz'), **out)
    print('reference script golden:', {k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    rng_kats()
    tacotron_shapes()
    only = sys.argv[1:]
    if not only or 'tacotron_decoder_200f' in only:
        tacotron_decoder_golden()
    if not only or 'tacotron_mirror' in only:
        tacotron_mirror_golden()
    if not only or 'reference_gen_wavernn' in only:
        reference_script_golden()
    for c in CASES:
        if only and c['name'] not in only:
            continue
        run_case(c)
