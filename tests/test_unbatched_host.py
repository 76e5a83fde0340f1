"""The host path of `batch.generate_unbatched` without a GPU: the C oracle stands in for the HIP loop (`loop_fn`), the chunks go through
`wrnn_post_chunk_host`.  Three random-weight utterances of 22, 24 and 21 frames, handed over unsorted, under 'cpu' seeds; the 24-frame one is the
utterance of tests/golden/{mol,raw}_unbatched_24f.npz -- what the reference's own unbatched `generate` returned for it.  CPU-only."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import MOL_TOL, case_mel, load_case, oracle_loop_fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 275
FRAMES = [22, 24, 21]                 # the caller's order: neither sorted nor reverse-sorted
GROUP_ORDER = [1, 0, 2]               # stable, longest first
CHUNK = 997

_SETUP = {}


def _setup(mode):
    """(model on the CPU, mels, seeds, mu_law, golden arrays, memoised oracle loop) of a mode, built once: the oracle is seconds of CPU per call, and
    several tests ask it for the same group"""
    if mode not in _SETUP:
        from wavernn_amd.model import WaveRNN
        from wavernn_amd.synthetic import SHIPPED, random_mel, random_state_dict
        cfg, g = load_case('mol_unbatched_24f' if mode == 'MOL' else 'raw_unbatched_24f')
        assert cfg['frames'] == 24 and not cfg['batched'] and cfg['mode'] == mode
        sd = random_state_dict(cfg['wseed'], mode=mode)
        model = WaveRNN(**SHIPPED, mode=mode)
        model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
        mels = [random_mel(701, 22), case_mel(cfg, g), random_mel(702, 21)]
        seeds = [311, cfg['seed'], 312]
        inner, memo = oracle_loop_fn(sd, mode), {}

        def loop_fn(mels_up, aux, seg_pos, seg_lim, T, noise, hop):
            h = hashlib.sha256()
            for a in (mels_up.numpy(), aux.numpy(), np.asarray(seg_pos), np.asarray(seg_lim), noise.numpy()):
                h.update(np.ascontiguousarray(a).tobytes())
            key = (h.hexdigest(), T, hop)
            if key not in memo:
                memo[key] = inner(mels_up, aux, seg_pos, seg_lim, T, noise, hop)
            return memo[key].clone()
        _SETUP[mode] = (model, mels, seeds, cfg['mu_law'], g, loop_fn)
    return _SETUP[mode]


_TOGETHER = {}


def _together(mode):
    """the three utterances in one chunked call, with its `on_chunk` record -- computed once, never modified"""
    if mode not in _TOGETHER:
        from wavernn_amd.batch import generate_unbatched
        model, mels, seeds, mu_law, g, loop_fn = _setup(mode)
        calls, tm = [], {}
        outs = generate_unbatched(model, mels, mu_law, seeds, noise_source='cpu', chunk_steps=CHUNK, loop_fn=loop_fn, timings=tm,
                                  on_chunk=lambda u, start, samples: calls.append((u, start, samples)))
        for o in outs:
            o.setflags(write=False)
        _TOGETHER[mode] = (outs, calls, tm)
    return _TOGETHER[mode]


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_results_come_back_in_the_callers_order_and_match_the_reference(mode):
    model, mels, seeds, mu_law, g, _ = _setup(mode)
    outs, _, tm = _together(mode)
    assert [o.shape for o in outs] == [((f - 1) * HOP,) for f in FRAMES] and all(o.dtype == np.float64 for o in outs)
    # the 24-frame utterance against what the reference's unbatched generate() returned after torch.manual_seed(seed): the bars of
    # test_oracle_golden.py / test_gpu_parity.py -- RAW identical, MoL within MOL_TOL
    if mode == 'RAW':
        assert np.array_equal(outs[1], g['out']), f'{np.count_nonzero(outs[1] != g["out"])} samples differ'
    else:
        assert np.abs(outs[1] - g['out']).max() <= MOL_TOL, np.abs(outs[1] - g['out']).max()
    assert tm['slices'] == -(-24 * HOP // CHUNK) and tm['first_chunk_ms'] > 0 and tm['loop_ms'] == 0.0


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_every_utterance_equals_the_same_function_on_it_alone(mode):
    from wavernn_amd.batch import generate_unbatched
    model, mels, seeds, mu_law, _, loop_fn = _setup(mode)
    outs, _, _ = _together(mode)
    for u in range(3):
        alone = generate_unbatched(model, [mels[u]], mu_law, [seeds[u]], noise_source='cpu', loop_fn=loop_fn)
        assert len(alone) == 1 and np.array_equal(alone[0], outs[u]), (u, np.abs(alone[0] - outs[u]).max())


@pytest.mark.parametrize('mode', ['MOL', 'RAW'])
def test_chunks_arrive_in_step_then_utterance_order_and_cover_every_sample_once(mode):
    outs, calls, _ = _together(mode)
    wave_len = [(f - 1) * HOP for f in FRAMES]
    expect = [(u, t0) for t0 in range(0, 24 * HOP, CHUNK) for u in GROUP_ORDER if t0 < wave_len[u]]
    assert [(u, start) for u, start, _ in calls] == expect
    for u in range(3):
        mine = [(start, s) for v, start, s in calls if v == u]
        assert all(len(s) == min(start + CHUNK, wave_len[u]) - start for start, s in mine)
        assert sum(len(s) for _, s in mine) == wave_len[u]
        assert np.array_equal(np.concatenate([s for _, s in mine]), outs[u])
        assert all(s.flags.owndata for _, s in mine)
    # copies, not views of one staging buffer: no two chunks share memory
    assert not any(np.shares_memory(a[2], b[2]) for i, a in enumerate(calls) for b in calls[i + 1:i + 4])


def test_max_utterances_cuts_groups_with_their_own_T():
    from wavernn_amd.batch import generate_unbatched, unbatched_groups
    assert unbatched_groups(FRAMES, 64) == [GROUP_ORDER] and unbatched_groups(FRAMES, 2) == [[1, 0], [2]]
    assert unbatched_groups([30, 21, 30, 25], 3) == [[0, 2, 3], [1]]                  # stable among equals
    model, mels, seeds, mu_law, _, loop_fn = _setup('MOL')
    outs, _, _ = _together('MOL')
    seen = []

    def spy(mels_up, aux, seg_pos, seg_lim, T, noise, hop):
        seen.append((len(seg_pos), T, [int(p) for p in seg_pos], [int(p) for p in seg_lim]))
        return loop_fn(mels_up, aux, seg_pos, seg_lim, T, noise, hop)
    calls = []
    two = generate_unbatched(model, mels, mu_law, seeds, noise_source='cpu', max_utterances=2, loop_fn=spy, dtype=np.float32,
                             on_chunk=lambda u, start, s: calls.append((u, start, len(s))))
    # group 0: 24 and 22 frames, T = 24 hops, each on a frame boundary of the concatenated conditioning; group 1: the 21-frame one with ITS T
    assert seen == [(2, 24 * HOP, [0, 24 * HOP], [24 * HOP, 46 * HOP]), (1, 21 * HOP, [0], [21 * HOP])]
    assert calls == [(1, 0, 23 * HOP), (0, 0, 21 * HOP), (2, 0, 20 * HOP)]            # unchunked: one chunk per utterance, group by group
    for u in range(3):
        assert two[u].dtype == np.float32 and np.array_equal(two[u], outs[u].astype(np.float32)), u


def test_short_mels_and_bad_arguments_raise_before_the_loop():
    from wavernn_amd.batch import generate_unbatched
    from wavernn_amd.synthetic import random_mel
    model, mels, seeds, mu_law, _, _ = _setup('MOL')

    def never(*a):
        raise AssertionError('the loop was reached')
    with pytest.raises(ValueError, match=r'operands could not be broadcast together with shapes \(5225,\) \(5500,\)'):
        generate_unbatched(model, [mels[0], random_mel(5, 20)], mu_law, [1, 2], noise_source='cpu', loop_fn=never)
    with pytest.raises(ValueError, match='needs `seeds`'):
        generate_unbatched(model, mels, mu_law, None, noise_source='library', loop_fn=never)
    with pytest.raises(ValueError, match='unknown noise source'):
        generate_unbatched(model, mels, mu_law, seeds, noise_source='gpu', loop_fn=never)
    with pytest.raises(ValueError):
        generate_unbatched(model, mels, mu_law, seeds[:2], noise_source='cpu', loop_fn=never)
    with pytest.raises(ValueError):
        generate_unbatched(model, mels, mu_law, seeds, noise_source='cpu', chunk_steps=0, loop_fn=never)
    with pytest.raises(ValueError):
        generate_unbatched(model, mels, mu_law, seeds, noise_source='cpu', dtype=np.float16, loop_fn=never)
    with pytest.raises(RuntimeError, match='HIP device'):                              # no loop_fn, model on the CPU: no quiet host path
        generate_unbatched(model, mels, mu_law, seeds, noise_source='cpu')


def test_library_noise_on_the_host_path_does_not_depend_on_the_group():
    """'library' noise through the stand-in (`wrnn_noise_fill_host` under the utterance's stream id): an utterance sounds the same alone and in a group."""
    from wavernn_amd.batch import generate_unbatched
    model, mels, _, mu_law, _, loop_fn = _setup('MOL')
    pair = generate_unbatched(model, [mels[2], mels[0]], mu_law, [7, 8], noise_source='library', loop_fn=loop_fn, chunk_steps=1651)
    alone = generate_unbatched(model, [mels[2]], mu_law, [7], noise_source='library', loop_fn=loop_fn)
    assert np.array_equal(pair[0], alone[0]) and pair[1].shape == (21 * HOP,)


def test_cli_argument_checks(tmp_path):
    from wavernn_amd import gen_tacotron
    a = gen_tacotron.parse_args(['--batch', '4', '--unbatched', '--tts_weights', 't.pyt', '--voc_weights', 'v.pyt', '--sentences', 's.txt'])
    assert a.batch == 4 and a.batched is False
    assert gen_tacotron.parse_args(['--batch', '4', '--tts_weights', 't.pyt', '--voc_weights', 'v.pyt']).batched is True
    assert 'needs --batched' not in open(gen_tacotron.__file__).read()
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', PYTHONPATH=os.pathsep.join([ROOT, os.environ.get('PYTHONPATH', '')]))
    r = subprocess.run([sys.executable, '-m', 'wavernn_amd.gen_corpus', '--mels', str(tmp_path), '--unbatched'], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode != 0 and 'gen_corpus --unbatched runs in a single process' in r.stderr, r.stderr[-2000:]
    from wavernn_amd import gen_corpus
    with pytest.raises(SystemExit):
        gen_corpus.main(['--mels', str(tmp_path), '--chunk-steps', '2200'])           # needs --unbatched
    src = open(gen_corpus.__file__).read()
    assert 'gen_NOT_BATCHED' in src
