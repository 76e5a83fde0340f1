"""`wrnn_pre_upsample_many` on the device (csrc/wrnn_pre.hip): four utterances in ONE call -- 1 frame (the smallest `wrnn_pre_upsample` accepts: n_frames >= 1,
include/wavernn_amd.h), 16 (exactly one 16-frame MelResNet tile), 17 (one frame past it) and 53 (ragged) -- both forms (the full up-sampled mel and the
`_rows` form), written into slices of one concatenated buffer with canary rows in front of, between and behind them.  Every slice equals, bit for bit,
what `wrnn_pre_upsample` / `_rows` write for that utterance alone, and no canary row is touched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES = (1, 16, 17, 53)
GUARD = 3                 # canary rows around every slice
CANARY = -7777.25


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available(), 'these tests need a HIP device'
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def case(gpu):
    """PreEngine, the mels, and the per-utterance results (`wrnn_pre_upsample` / `_rows`, one call each): computed once."""
    from wavernn_amd.pre import PreEngine
    from wavernn_amd.synthetic import random_mel, random_state_dict
    pre = PreEngine(random_state_dict(31, mode='MOL'), device=gpu)
    mels = [torch.from_numpy(random_mel(1700 + k, n)).to(gpu) for k, n in enumerate(FRAMES)]
    ref = {False: [tuple(t.cpu().numpy() for t in pre.upsample(m)) for m in mels],
           True: [tuple(t.cpu().numpy() for t in pre.upsample_rows(m)) for m in mels]}
    torch.cuda.synchronize()
    return pre, mels, ref


@pytest.mark.parametrize('rows', [False, True], ids=['full', 'rows'])
def test_many_equals_one_by_one_and_keeps_the_canaries(gpu, case, rows):
    from wavernn_amd import _lib
    pre, mels, ref = case
    L = _lib.lib()
    n_up = [pre.rows_of(n) if rows else n * pre.hop for n in FRAMES]
    tab = (_lib.PreUtt * len(FRAMES))()
    r, a = GUARD, GUARD
    for k, n in enumerate(FRAMES):
        tab[k].mel, tab[k].n_frames, tab[k].up_row, tab[k].aux_row = mels[k].data_ptr(), n, r, a
        r, a = r + n_up[k] + GUARD, a + n + GUARD
    up = torch.full((r, 80), CANARY, dtype=torch.float32, device=gpu)
    aux = torch.full((a, 128), CANARY, dtype=torch.float32, device=gpu)
    nbytes = int(L.wrnn_pre_workspace_bytes_many(pre._pre, tab, len(FRAMES), int(rows)))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    rc = L.wrnn_pre_upsample_many(pre._pre, tab, len(FRAMES), int(rows), up.data_ptr(), aux.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.wrnn_pre_last_error()
    torch.cuda.synchronize()
    up, aux = up.cpu().numpy(), aux.cpu().numpy()
    canary_up, canary_aux = np.ones(len(up), bool), np.ones(len(aux), bool)
    for k, n in enumerate(FRAMES):
        r0, a0 = int(tab[k].up_row), int(tab[k].aux_row)
        want_up, want_aux = ref[rows][k]
        assert want_up.shape == (n_up[k], 80) and want_aux.shape == (n, 128)
        assert np.array_equal(up[r0:r0 + n_up[k]], want_up), f'utterance {k} ({n} frames): mel differs from the per-utterance call'
        assert np.array_equal(aux[a0:a0 + n], want_aux), f'utterance {k} ({n} frames): aux differs from the per-utterance call'
        canary_up[r0:r0 + n_up[k]] = False
        canary_aux[a0:a0 + n] = False
    assert canary_up.sum() == GUARD * (len(FRAMES) + 1) and canary_aux.sum() == GUARD * (len(FRAMES) + 1)
    assert (up[canary_up] == CANARY).all() and (aux[canary_aux] == CANARY).all(), 'a canary row was written'


@pytest.mark.parametrize('rows', [False, True], ids=['full', 'rows'])
def test_upsample_many_paths_agree(gpu, case, rows):
    """The Python face: `PreEngine.upsample_many` batched (here: streams = 0), one by one (1) and on side streams (2) fill the same views with the same bits."""
    pre, mels, ref = case
    got = {}
    for streams in (0, 1, 2):
        n_up = [pre.rows_of(n) if rows else n * pre.hop for n in FRAMES]
        up = torch.zeros(sum(n_up), 80, dtype=torch.float32, device=gpu)
        aux = torch.zeros(sum(FRAMES), 128, dtype=torch.float32, device=gpu)
        jobs, r, a = [], 0, 0
        for m, n, nu in zip(mels, FRAMES, n_up):
            jobs.append((m, up[r:r + nu], aux[a:a + n]))
            r, a = r + nu, a + n
        pre.upsample_many(jobs, rows=rows, streams=streams, batched=streams == 0)
        torch.cuda.synchronize()
        got[streams] = (up.cpu().numpy(), aux.cpu().numpy())
    want = tuple(np.concatenate([ref[rows][k][i] for k in range(len(FRAMES))]) for i in (0, 1))
    for streams in (0, 1, 2):
        assert np.array_equal(got[streams][0], want[0]) and np.array_equal(got[streams][1], want[1]), streams
