"""Corpus-level batched generation: many utterances -> one segment table -> shards over ranks -> all-gather.

The reference generates one utterance per `WaveRNN.generate()` call (gen_wavernn.py:26-35, :56-65): each call
folds ITS mel into `num_folds` overlapping segments (models/fatchord_version.py:293-340), runs them as one batch
and cross-fades them back (:342-405).  Folded segments are independent from step 0 (zero initial state,
:194-196; no cross-segment term in :201-241), so the segments of SEVERAL utterances can share one launch, and a
corpus can be cut into contiguous blocks of segments, one block per GPU (BASELINE config
4).  This module is the host logic for that:

  plan_utterances   the segment table (`seg_pos`, `seg_lim`) over the concatenated conditioning
  shard_bounds      contiguous, balanced blocks of segments per rank (no data-path collective inside the loop)
  pack_noise        per-utterance reference noise streams -> the launch's [T, 11*n] / [T, n, C] layout
  generate_corpus   upsample (PyTorch) -> loop (libwavernn_amd.so) on this rank's block -> all_gather of the
                    [n_r, T] audio (RCCL over xGMI when the process group is `nccl`) -> per-utterance unfold

Results do not depend on the number of ranks: every segment's noise is addressed by (utterance seed, step, fold
index) exactly as the single-utterance reference call would draw it.
"""
import time
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import fold as _fold


@dataclass
class Plan:
    target: int
    overlap: int
    T: int                    # steps per segment = target + 2*overlap
    stride: int               # target + overlap
    lengths: List[int]        # un-folded conditioning length (samples) of every utterance
    offsets: np.ndarray       # sample offset of every utterance in the concatenated conditioning
    folds: np.ndarray         # segments per utterance (num_folds of fold_with_overlap)
    first: np.ndarray         # index of every utterance's first segment
    seg_pos: np.ndarray       # int32 [n_segments]: conditioning position of step 0
    seg_lim: np.ndarray       # int32 [n_segments]: first position that is zero padding (the utterance's end)
    seg_utt: np.ndarray       # int32 [n_segments]: owning utterance

    @property
    def n_segments(self):
        return int(self.seg_pos.shape[0])

    @property
    def total_len(self):
        return int(sum(self.lengths))


def plan_utterances(lengths: Sequence[int], target: int, overlap: int) -> Plan:
    """Segment table for utterances whose un-folded conditioning (lengths[u] samples each) is concatenated."""
    lengths = [int(x) for x in lengths]
    if not lengths or min(lengths) < 1:
        raise ValueError('need at least one non-empty utterance')
    stride, T = target + overlap, target + 2 * overlap
    folds = np.array([_fold.fold_geometry(L, target, overlap)[0] for L in lengths], dtype=np.int64)
    # reference quirk: an input shorter than one window still makes one zero-padded fold (:322-330)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(folds)[:-1]]).astype(np.int64)
    if offsets[-1] + lengths[-1] + T >= 2 ** 31:
        raise ValueError('concatenated conditioning exceeds int32 positions; split the corpus')
    seg_pos, seg_lim, seg_utt = [], [], []
    for u, (L, nf) in enumerate(zip(lengths, folds)):
        seg_pos.append(offsets[u] + np.arange(nf, dtype=np.int64) * stride)
        seg_lim.append(np.full(nf, offsets[u] + L, dtype=np.int64))
        seg_utt.append(np.full(nf, u, dtype=np.int64))
    return Plan(target, overlap, T, stride, lengths, offsets, folds, first,
                np.concatenate(seg_pos).astype(np.int32), np.concatenate(seg_lim).astype(np.int32),
                np.concatenate(seg_utt).astype(np.int32))


def shard_bounds(n_segments: int, world: int, active: Optional[int] = None):
    """[(lo, hi)] * world: contiguous blocks whose sizes differ by at most one (block r = segments [lo, hi)).  active < world: only the
    first `active` ranks get a block (`choose_ranks`); the others own the empty block (n, n) and only take part in the all-gather."""
    active = world if active is None else max(1, min(int(active), world))
    return [((r * n_segments) // active, ((r + 1) * n_segments) // active) if r < active else (n_segments, n_segments) for r in range(world)]


#: LAST-RESORT step times (us) of the dense MoL loop kernels by groups in flight per cluster (4 clusters x depth x 16 segments per GPU, one MI355X,
#: round 6: wrnn_chain_kernel at depth 1-2, wrnn_duo_kernel from 3 on).  `choose_ranks` plans with a table that is MEASURED: bench.py times the
#: depths on the device it runs on and hands the table over (and records it in profiles/step_us.json, keyed by a hash of the kernel sources, like
#: profiles/traffic_latest.json); without one `step_table()` reads that file and falls back to these numbers -- saying so -- only when the file is
#: missing or was measured on other sources.
DEFAULT_STEP_US_BY_DEPTH = {1: 10.4, 2: 13.8, 3: 19.4, 4: 22.9, 5: 27.4, 6: 31.3, 7: 35.5, 8: 38.9}
_STEP_TABLE = None


def kernel_source_sha16() -> str:
    """Hash of the sources the dense loop kernels are compiled from (what a measured step-time / traffic record belongs to)."""
    import hashlib
    import os
    from . import _lib
    h = hashlib.sha256()
    for name in ('wrnn_abi.hip', 'wrnn_cond.hip', 'wrnn_device.h', 'wrnn_duo.hip', 'wrnn_loop.hip', 'wrnn_ring.h', 'wrnn_tiles.h'):
        h.update(open(os.path.join(_lib.CSRC, name), 'rb').read())
    return h.hexdigest()[:16]


def step_table(path: Optional[str] = None):
    """(table {depth: us per step}, origin string).  The record bench.py wrote for THESE kernel sources, else the built-in numbers."""
    global _STEP_TABLE
    if _STEP_TABLE is None or path is not None:
        import json
        import os
        from . import _lib
        f = path or os.path.join(os.path.dirname(os.path.dirname(_lib.CSRC)), 'profiles', 'step_us.json')
        table, origin = dict(DEFAULT_STEP_US_BY_DEPTH), 'built-in defaults (no profiles/step_us.json)'
        try:
            j = json.load(open(f))
            if j.get('source_sha16') == kernel_source_sha16():
                table, origin = {int(k): float(v) for k, v in j['step_us_by_depth'].items()}, f'{f} (measured on these kernel sources)'
            else:
                origin = f'built-in defaults ({f} was measured on other kernel sources)'
        except (OSError, ValueError, KeyError):
            pass
        if path is not None:
            return table, origin
        _STEP_TABLE = (table, origin)
    return _STEP_TABLE


def estimate_step_us(n_segments: int, table: Optional[dict] = None) -> float:
    """Step time of one GPU that advances `n_segments` segments by one sample (rounds of <= 512 segments at the measured depth)."""
    if n_segments <= 0:
        return 0.0
    table = table or step_table()[0]
    groups = -(-n_segments // 16)
    rounds = -(-groups // 32)
    depth = min(8, max(1, -(-(-(-groups // rounds)) // 4)))
    return rounds * table[depth]


def choose_ranks(n_segments: int, world: int, table: Optional[dict] = None) -> int:
    """How many of `world` GPUs a FIXED corpus of `n_segments` folded segments should be sharded over (strong scaling, BASELINE config 4):
    the wall time of a pass is the step time of the largest block, which depends on the pipeline depth that block fills -- not on the rank
    count as such -- so the smallest rank count that reaches the best estimated wall time is taken (942 segments on 8 GPUs: 118 per GPU =
    depth 2, and 7 GPUs would need depth 3: all 8; on 16 GPUs: 15 suffice).  The ranks left out still take part in the all-gather.
    table: {depth: us per step} measured by the caller (bench.py); default: `step_table()`."""
    est = [estimate_step_us(-(-n_segments // r), table) for r in range(1, world + 1)]
    best = min(est)
    return 1 + next(i for i, e in enumerate(est) if e <= best * 1.01)


def pack_noise(mode: str, plan: Plan, per_utt, lo: int = 0, hi: Optional[int] = None, steps: Optional[int] = None):
    """Arrange per-utterance noise into the layout `wrnn_generate_segments` reads for segments [lo, hi).

    per_utt[u] is utterance u's noise exactly as the reference draws it for that utterance alone: MOL
    (T, 11*B_u) = per step 10*B_u mixture uniforms (segment-major) then B_u logistic uniforms; RAW (T, B_u, C).
    Entries for utterances without a segment in [lo, hi) may be None.  numpy in -> numpy out, torch in -> torch out.
    steps: the rows are a slice of `steps` consecutive loop steps instead of all plan.T (a step-sliced run).
    """
    hi = plan.n_segments if hi is None else hi
    T = plan.T if steps is None else int(steps)
    n = hi - lo
    utts = [u for u in range(len(plan.lengths)) if plan.first[u] < hi and plan.first[u] + plan.folds[u] > lo]
    sample = per_utt[utts[0]]
    is_torch = isinstance(sample, torch.Tensor)
    cat = (lambda xs, d: torch.cat(xs, dim=d)) if is_torch else (lambda xs, d: np.concatenate(xs, axis=d))
    mix, logi, raw = [], [], []
    for u in utts:
        Bu, f0 = int(plan.folds[u]), int(plan.first[u])
        a, b = max(lo, f0) - f0, min(hi, f0 + Bu) - f0          # this utterance's segments [a, b) are in the block
        z = per_utt[u]
        if mode == 'MOL':
            z = z.reshape(T, 11 * Bu)
            mix.append(z[:, 10 * a:10 * b])
            logi.append(z[:, 10 * Bu + a:10 * Bu + b])
        else:
            raw.append(z.reshape(T, Bu, -1)[:, a:b])
    out = cat(mix + logi, 1) if mode == 'MOL' else cat(raw, 1)
    assert out.shape[0] == T and (out.shape[1] == 11 * n if mode == 'MOL' else out.shape[1] == n)
    return out.contiguous() if is_torch else np.ascontiguousarray(out)


def library_seg_ids(seed, folds, first_fold: int = 0) -> np.ndarray:
    """The 64-bit noise stream ids (wrnn_options.noise_seg_id) of `folds` consecutive folded segments of ONE utterance, from its fold `first_fold` on:
    (seed & 0xffffffff) << 32 | fold index.  What `WaveRNN.generate()` (seed = model.noise_seed) and `generate_corpus(noise_source='library')`
    (seed = seeds[u]) both use -- the reason an utterance's audio does not depend on the batch, chunk or shard it was generated in."""
    hi = np.uint64((int(seed) & 0xffffffff) << 32)
    return hi | np.arange(first_fold, first_fold + int(folds), dtype=np.uint64)


def chunk_utterances(plan: Plan, lo: int, hi: int, max_segments: int):
    """Cut the utterances that own segments in [lo, hi) into consecutive chunks whose segment count in [lo, hi) stays
    <= max_segments (a single longer utterance makes its own chunk).  Returns [(utterances, seg_lo, seg_hi)]."""
    chunks, cur, cur_lo, cur_hi = [], [], None, None
    for u in range(len(plan.lengths)):
        a, b = max(lo, int(plan.first[u])), min(hi, int(plan.first[u] + plan.folds[u]))
        if a >= b:
            continue
        if cur and (b - cur_lo) > max_segments:
            chunks.append((cur, cur_lo, cur_hi))
            cur, cur_lo = [], None
        if cur_lo is None:
            cur_lo = a
        cur.append(u)
        cur_hi = b
    if cur:
        chunks.append((cur, cur_lo, cur_hi))
    return chunks


def score_corpus(model, mels: Sequence, wavs: Sequence, mu_law: Optional[bool] = None, per_step: bool = False, algo: Optional[str] = None,
                 timings: Optional[dict] = None):
    """Teacher-forced negative log-likelihood of n utterances (`score.score_corpus`): they become the n unfolded segments of ONE segment table per
    chunk -- seg_pos = o_u, seg_lim = o_u + the utterance's counted steps, T = the longest --, run by one loop call with `force_x` and `logits`
    and scored by one `wrnn_nll` launch on the same stream.  Chunks keep the logits under `model.score_logits_bytes`; the results come back in
    the caller's order."""
    from .score import score_corpus as _score_corpus
    return _score_corpus(model, mels, wavs, mu_law=mu_law, per_step=per_step, algo=algo, timings=timings)


def generate_corpus(model, mels: Sequence, target: int, overlap: int, mu_law: bool, seeds: Optional[Sequence[int]] = None,
                    group=None, loop_fn=None, return_segments=False, noise_source='cpu', finish='all', check=True,
                    max_segments_per_launch: int = 4096, shard=None, ranks: Optional[int] = None, timings: Optional[dict] = None):
    """Generate every utterance of `mels` (each (1, feat, N_u) or (feat, N_u)) with `model` (a `wavernn_amd.WaveRNN`),
    batched, sharding the folded segments over the ranks of `group` (None = single process).

    seeds[u] plays the role of `torch.manual_seed(seeds[u])` before the reference's `generate()` call for utterance u
    (parity noise: the CPU MT19937 stream incl. the GRUCell constructor draws).  Returns the list of float64 waveforms
    (on every rank), equal to per-utterance `generate(mel_u, ..., batched=True, target, overlap, mu_law)` calls.

    noise_source='device' draws the block's noise from the device generator instead (what the reference does when it
    runs on a GPU; not comparable with a CPU run; `seeds` unused).  noise_source='library': the loop draws its noise itself
    (wrnn_options.noise_lib; key `model.noise_key`), segment `i` of utterance u under the stream id `library_seg_ids(seeds[u], ...)`: one engine
    call per chunk, no noise tensor, and every utterance equal to `generate()` alone with `model.noise_source = 'library'` and
    `model.noise_seed = seeds[u]`, whatever the chunking and the rank count.  finish='all': every rank unfolds every utterance;
    'own': a rank unfolds only the utterances whose first segment lies in its block (None elsewhere in the list).

    The rank's block is processed in chunks of whole utterances of at most `max_segments_per_launch` segments, so the
    conditioning (320 B per audio sample) and the sampling noise of only one chunk are resident at a time; the loop's own
    workspace does not grow with the corpus (conditioning slabs, `wrnn_workspace_bytes_segments`).

    shard=(r, w), without a group: do what rank r of a w-rank job does on its own -- its block of the segment table, the post-loop
    stage of the utterances lying entirely in it -- with no collective (how bench.py shows a GPU's share of config 4 at N = 1).

    ranks: shard over the first `ranks` ranks of the group only (`choose_ranks`; None = all).  timings: optional dict, filled with
    `gather_wait_ms` (host time blocked on the all-gather) and `unfold_under_gather_ms` (post-loop stage of this rank's own utterances,
    run while the gather is in flight).

    loop_fn(mels_up, aux, seg_pos, seg_lim, T, noise, hop) -> (n, T) tensor replaces the HIP loop (tests inject a CPU
    stand-in to exercise the sharding / gather logic under gloo); the default is the model's LoopEngine.
    """
    import torch.distributed as dist
    from .rng import draw_steps
    if noise_source in ('cpu', 'library') and seeds is None:
        raise ValueError(f"noise_source={noise_source!r} needs `seeds` (one per utterance); "
                         "pass noise_source='device' to draw from the device generator instead")
    if noise_source not in ('cpu', 'device', 'library'):
        raise ValueError(f'unknown noise source {noise_source!r}')
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    if shard is not None:
        if group is not None:
            raise ValueError('shard=(rank, world) emulates a rank without a process group')
        rank, world = int(shard[0]), int(shard[1])
        finish = 'own'
    device = next(model.parameters()).device
    mode = model.mode
    mu_law = mu_law if mode == 'RAW' else False
    hop = model.hop_length
    was_training = model.training
    model.eval()
    mels = [torch.as_tensor(m) for m in mels]
    mels = [m.unsqueeze(0) if m.dim() == 2 else m for m in mels]
    frames = [int(m.size(-1)) for m in mels]
    plan = plan_utterances([n * hop for n in frames], target, overlap)
    bounds = shard_bounds(plan.n_segments, world, ranks)
    lo, hi = bounds[rank]
    n_max = max(h - l for l, h in bounds)

    out_local = torch.zeros(n_max, plan.T, dtype=torch.float32, device=device)
    native_pre = loop_fn is None and getattr(model, 'pre_algo', 'torch') == 'native' and device.type == 'cuda'
    # the post-loop stage's share of the utterances is known from the plan: its tables go to the device now, in front of the loop, so that
    # nothing but the unfold launch and the copy to the host follows the last loop launch (model.post_tables_early = False: behind the loop, A/B)
    n_utt = len(frames)
    mine_u = [u for u in range(n_utt) if finish != 'own' or (lo <= plan.first[u] < hi)]
    local_u = [u for u in mine_u if lo <= plan.first[u] and plan.first[u] + plan.folds[u] <= hi]      # no segment on another rank
    local_set = set(local_u)
    rest_u = [u for u in mine_u if u not in local_set]
    native_post = loop_fn is None and getattr(model, 'post_algo', 'numpy') == 'native' and out_local.is_cuda
    slab_tuning = 8192 if getattr(model, 'slab_prep_split', False) else 0       # (wrnn_options.tuning bit 13: the three-call slab preparation, A/B)

    def unfold_args(us, first_of):
        return ([first_of(u) for u in us], [int(plan.folds[u]) for u in us], [(frames[u] - 1) * hop for u in us], overlap, hop, model.n_classes, mu_law, True)
    first_local, first_all = (lambda u: int(plan.first[u]) - lo), (lambda u: int(plan.first[u]))
    early = {}
    if native_post and not return_segments and getattr(model, 'post_tables_early', True):
        from .post import prepare_unfold
        for us, first_of in ((local_u, first_local), (rest_u, first_all)):
            if us and not (shard is not None and first_of is first_all):
                early[first_of] = prepare_unfold(*unfold_args(us, first_of), device=device)
    with torch.no_grad():
        for utts, clo, chi in (chunk_utterances(plan, lo, hi, max_segments_per_launch) if hi > lo else []):
            # conditioning of the utterances this chunk touches, concatenated (each starts on a frame boundary)
            noise = [None] * len(mels)
            local_off, off = {}, 0
            for u in utts:
                local_off[u] = off
                off += frames[u] * hop
            n_seg, T = chi - clo, plan.T
            eng = model._loop_engine() if loop_fn is None else None

            def conditioning(rows):
                """rows: the mel one up-sampling stage short (`engine.MelRows`; wrnn_duo_kernel forms the last stage in the loop)"""
                if native_pre:     # the pre-loop kernels write straight into their slices of the concatenated buffers
                    pre = model._pre_engine()
                    n_rows = [pre.rows_of(frames[u]) for u in utts] if rows else None
                    mels_up = torch.empty(sum(n_rows) if rows else off, mels[utts[0]].size(1), dtype=torch.float32, device=device)
                    aux = torch.empty(off // hop, 4 * model.aux_dims, dtype=torch.float32, device=device)
                    r0, jobs = 0, []
                    for k, u in enumerate(utts):
                        a0 = local_off[u]
                        if rows:
                            jobs.append((mels[u], mels_up[r0:r0 + n_rows[k]], aux[a0 // hop:a0 // hop + frames[u]]))
                            r0 += n_rows[k]
                        else:
                            jobs.append((mels[u], mels_up[a0:a0 + frames[u] * hop], aux[a0 // hop:a0 // hop + frames[u]]))
                    pre.upsample_many(jobs, rows=rows, streams=int(getattr(model, 'pre_streams', 8)),
                                      batched=bool(getattr(model, 'pre_batched', True)))      # (batched: one launch per stage for all of them)
                    if rows:       # utterance k of the chunk: its rows start 2 * indent * k samples later than its cropped samples do
                        from .engine import MelRows
                        indent, order = pre.pad * hop, {u: k for k, u in enumerate(utts)}
                        seg_off = np.array([indent * (2 * order[int(u)] + 1) for u in plan.seg_utt[clo:chi]], dtype=np.int32)
                        mels_up = MelRows(mels_up, off, pre.scales[2], pre.last_taps, seg_off)
                    return mels_up, aux
                ups, auxs = zip(*[model.conditioning(mels[u])[:2] for u in utts])
                return torch.cat(ups).contiguous(), torch.cat(auxs).contiguous()
            rows = eng is not None and native_pre and model.mel_rows_ok(eng, n_seg, T)
            mels_up, aux = conditioning(rows)
            # this chunk's segment table, rebased onto the conditioning of the utterances it touches
            rebase = np.array([local_off[int(u)] - int(plan.offsets[int(u)]) for u in plan.seg_utt[clo:chi]], dtype=np.int64)
            seg_pos = (plan.seg_pos[clo:chi].astype(np.int64) + rebase).astype(np.int32)
            seg_lim = (plan.seg_lim[clo:chi].astype(np.int64) + rebase).astype(np.int32)
            out_view = out_local[clo - lo:chi - lo]
            # the reference's per-utterance CPU streams (parity noise): one private generator per utterance, the GRUCell constructor
            # draws burnt once, then the loop's draws in step order -- so a slice of steps continues every stream where the last stopped
            gens, pool = {}, None
            if noise_source == 'cpu':
                if len(utts) > 1 and mode == 'RAW':       # (MoL: 11 draws per segment-step -- not worth a thread)
                    import os
                    from concurrent.futures import ThreadPoolExecutor
                    # (the host's cores are shared by the ranks of the node: LOCAL_WORLD_SIZE, as torch.distributed.run and bench.py set it)
                    pool = ThreadPoolExecutor(max(1, min(len(utts), (os.cpu_count() or 2) // (2 * max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1')))))))
                from .rng import burn_ctor_draws
                for u in utts:
                    gens[u] = torch.Generator(device='cpu').manual_seed(int(seeds[u]))
                    burn_ctor_draws(model.rnn_dims, model.aux_dims, 'cpu', gens[u])

            lib_ids = None
            if noise_source == 'library':
                lib_ids = np.concatenate([library_seg_ids(seeds[u], min(chi, int(plan.first[u] + plan.folds[u])) - max(clo, int(plan.first[u])),
                                                          max(clo, int(plan.first[u])) - int(plan.first[u])) for u in utts])
                assert lib_ids.shape == (n_seg,)
            lib_kw = dict(noise_seed=int(getattr(model, 'noise_key', 0)), noise_seg_id=lib_ids) if lib_ids is not None else {}

            def draw(steps_):
                """noise rows of the next `steps_` loop steps of this chunk's segments, on the device"""
                if noise_source == 'library':
                    if loop_fn is None:
                        return None              # (the loop draws it)
                    from ._lib import noise_fill_host
                    return torch.from_numpy(noise_fill_host(mode, n_seg, model.n_classes, 0, steps_, lib_kw['noise_seed'], lib_ids)).to(device)
                if noise_source != 'cpu':
                    return draw_steps(mode, n_seg, steps_, model.n_classes, device, 'device')
                def one(u):        # (ATen releases the GIL inside the fill: the utterances' independent streams are drawn side by side)
                    noise[u] = draw_steps(mode, int(plan.folds[u]), steps_, model.n_classes, 'cpu', 'cpu', generator=gens[u])
                if pool is None:
                    for u in utts:
                        one(u)
                else:
                    list(pool.map(one, utts))
                return pack_noise(mode, plan, noise, clo, chi, steps=steps_).to(device)

            if loop_fn is not None:
                out_view[:] = loop_fn(mels_up, aux, seg_pos, seg_lim, T, draw(T), hop)
                if pool is not None:
                    pool.shutdown()
                continue
            from ._lib import ResidencyError
            from .engine import RESUMABLE_KERNELS
            # the persistent loop kernels continue a call (wrnn_options.t_begin / t_end): the noise -- RAW: n_classes floats per
            # segment-step -- is drawn and uploaded in slices of steps, at most `model.noise_chunk_bytes` of it resident (the bound
            # WaveRNN.generate() keeps); any other kernel takes the whole call's noise at once
            steps = T
            groups = model.loop_sparse_groups(eng, n_seg, T) if hasattr(model, 'loop_sparse_groups') else 0      # (model.sparse_groups; 0 unless wrnn_sparse_kernel is planned)
            if noise_source != 'library' and eng.plan(n_seg, T, algo=model.loop_algo)['kernel'] in RESUMABLE_KERNELS:
                per_step = n_seg * (11 if mode == 'MOL' else model.n_classes) * 4
                steps = max(1, min(T, getattr(model, 'noise_chunk_bytes', 2 << 30) // per_step))
                steps = -(-T // (-(-T // steps)))            # equal slices (no short tail slice with its own launches)
            try:
                for t0 in range(0, T, steps):
                    t1 = min(T, t0 + steps)
                    eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, draw(t1 - t0), hop, algo=model.loop_algo, check=check, out=out_view,
                                     t_range=None if (t0 == 0 and t1 == T) else (t0, t1), sparse_groups=groups, tuning=slab_tuning, **lib_kw)
            except ResidencyError as e:
                # the persistent grid was refused (on the first slice: a continuation cannot change kernels).  The other loop kernels read
                # the up-sampled mel in full; the engine then degrades as usual on an unsliced call (one workgroup per CU, then the
                # stream kernel), from the start of every utterance's noise stream
                import warnings
                warnings.warn(f'wavernn_amd: {e}; redoing the chunk unsliced on the next kernel')
                if rows:
                    mels_up, aux = conditioning(False)
                for u in gens:
                    gens[u].manual_seed(int(seeds[u]))
                    burn_ctor_draws(model.rnn_dims, model.aux_dims, 'cpu', gens[u])
                eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, draw(T), hop, algo=model.loop_algo, check=check, out=out_view, sparse_groups=groups, tuning=slab_tuning, **lib_kw)
            finally:
                if pool is not None:
                    pool.shutdown()
    # ---- the ONE collective of the path: an all-gather of the finished audio, asynchronous so that the utterances lying entirely in
    #      this rank's block are unfolded (post-loop stage) while the other ranks' segments are still on their way over xGMI
    n_utt = len(frames)
    work, gathered = None, None
    if group is not None:
        gathered = [torch.empty_like(out_local) for _ in range(world)]
        work = dist.all_gather(gathered, out_local, group=group, async_op=True)
        if timings is not None:                         # what this rank receives over the fabric in the ONE collective of the path
            timings['gather_bytes'] = timings.get('gather_bytes', 0) + (world - 1) * out_local.numel() * out_local.element_size()
            timings['world_seen'] = dist.get_world_size(group)

    def gathered_segments():
        nonlocal work
        if group is None:
            if shard is not None:
                raise ValueError('an emulated shard has only its own block of segments')
            return out_local[:plan.n_segments]
        if work is not None:
            t_w = time.perf_counter()
            work.wait()
            work = None
            if timings is not None:
                timings['gather_wait_ms'] = timings.get('gather_wait_ms', 0.0) + (time.perf_counter() - t_w) * 1e3
        return torch.cat([gathered[r][:h - l] for r, (l, h) in enumerate(bounds)])

    if was_training:
        model.train()
    if return_segments:
        return gathered_segments().cpu().numpy().astype(np.float64), plan
    outs = [None] * n_utt

    def unfold(segs, first_of, us):
        """Post-loop stage (reference :245-260, :342-405) of utterances `us`, whose first segment is row first_of(u) of `segs`."""
        if not us:
            return
        if native_post:       # on the device (float64, reference order): one launch for all of them
            from .post import unfold_on_device
            wav, sl = unfold_on_device(segs, *unfold_args(us, first_of), tables=early.get(first_of))
            if getattr(model, 'pinned_output', True):
                # the finished audio (8 B per sample) into page-locked memory at the link's rate (a pageable copy is staged through bounce buffers);
                # torch's caching host allocator hands the pages back to the next call; the returned arrays are views that keep the buffer alive
                host = torch.empty(wav.shape, dtype=wav.dtype, pin_memory=True)
                host.copy_(wav, non_blocking=True)
                torch.cuda.current_stream(wav.device).synchronize()
                wav = host.numpy()
            else:
                wav = wav.cpu().numpy()
            for (a, b), u in zip(sl, us):
                outs[u] = wav[a:b]
            return
        host = segs.cpu().numpy().astype(np.float64)
        for u in us:
            y = host[first_of(u):first_of(u) + int(plan.folds[u])].copy()
            if mu_law:
                y = _fold.decode_mu_law(y, model.n_classes, False)
            y = _fold.xfade_and_unfold(y, target, overlap)
            outs[u] = _fold.finish_waveform(y, (frames[u] - 1) * hop, hop)

    t_u = time.perf_counter()
    unfold(out_local, first_local, local_u)          # under the all-gather
    if timings is not None:
        timings['unfold_under_gather_ms'] = timings.get('unfold_under_gather_ms', 0.0) + (time.perf_counter() - t_u) * 1e3
    if shard is not None:
        return outs
    if rest_u:
        unfold(gathered_segments(), first_all, rest_u)
    elif work is not None:
        t_w = time.perf_counter()
        work.wait()
        if timings is not None:
            timings['gather_wait_ms'] = timings.get('gather_wait_ms', 0.0) + (time.perf_counter() - t_w) * 1e3
    return outs


# ---- unbatched generation of a LIST of utterances: one unfolded segment each, one segment table per group, optionally streamed in step slices ----
def _unbatched_plan(frames, hop) -> Plan:
    """The one-fold-per-utterance plan of a group (what `pack_noise` reads): utterance k is segment k, frames[k] * hop conditioning positions from
    o_k on, T = the longest."""
    lengths = [int(f) * hop for f in frames]
    n, T = len(lengths), max(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    if int(off[-1]) + lengths[-1] + T >= 2 ** 31:
        raise ValueError('concatenated conditioning exceeds int32 positions; lower max_utterances')
    idx = np.arange(n, dtype=np.int64)
    return Plan(T, 0, T, T, lengths, off, np.ones(n, np.int64), idx, off.astype(np.int32), (off + np.asarray(lengths)).astype(np.int32), idx.astype(np.int32))


def unbatched_groups(frames: Sequence[int], max_utterances: int):
    """Utterance indices sorted by frame count -- stable, longest first -- and cut into groups of at most `max_utterances`."""
    order = sorted(range(len(frames)), key=lambda u: -int(frames[u]))
    return [order[i:i + max_utterances] for i in range(0, len(order), max_utterances)]


def _cut(t0, t1, bound):
    """[t0, t1) in equal pieces of at most `bound` steps."""
    pieces = -(-(t1 - t0) // max(1, bound))
    size = -(-(t1 - t0) // pieces)
    return [(a, min(t1, a + size)) for a in range(t0, t1, size)]


def live_release(slices, done, m):
    """The scheduling decision of the live path (`generate_unbatched(live=True)`): `slices` are the step ranges [t0, t1) of a call in delivery order, the
    first `done` of them have been released, and the loop kernel has just been seen to have finished steps [0, m).  Returns the new count: the slices
    [done, result) are released now, in order.  A slice is released only when m covers it (t1 <= m), never twice and never out of order, whatever the
    sequence of observations -- repeated, stuck, no multiple of the chunk, or running backwards; m = T releases everything."""
    k = int(done)
    while k < len(slices) and slices[k][1] <= m:
        k += 1
    return k


_WARNED_WHOLE = 'wavernn_amd: chunk_steps asks for step slices, but {} does not continue a call (engine.RESUMABLE_KERNELS): the call runs whole and ' \
                'every utterance is delivered as one chunk at the end'


def unbatched_chunks(model, mels: Sequence, mu_law: bool, seeds: Optional[Sequence[int]] = None, noise_source='library', chunk_steps: Optional[int] = None,
                     max_utterances: int = 64, dtype=np.float64, loop_fn=None, check=True, timings: Optional[dict] = None, global_rng=False, live=False):
    """The core of `generate_unbatched` and `WaveRNN.generate_stream`, as a generator of (u, start, samples): utterance u's finished samples
    [start, start + len(samples)), in step order and, within a step slice, in the group's order; `samples` is an array of its own.  While the
    generator is suspended the device goes on with the slice queued behind the one just delivered.  global_rng (one utterance, 'cpu' noise): draw
    from torch's global generator as `WaveRNN.generate` does, instead of a private generator seeded with seeds[u].  live: `generate_unbatched`."""
    from .rng import draw_steps, burn_ctor_draws
    from . import _lib
    from . import post as _post
    from .engine import RESUMABLE_KERNELS, WATCHABLE_KERNELS
    t_call = time.perf_counter()
    if noise_source not in ('cpu', 'device', 'library'):
        raise ValueError(f'unknown noise source {noise_source!r}')
    if noise_source in ('cpu', 'library') and seeds is None and not (global_rng and noise_source == 'cpu'):
        raise ValueError(f"noise_source={noise_source!r} needs `seeds` (one per utterance); pass noise_source='device' to draw from the device generator instead")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError('dtype: np.float64 or np.float32')
    if chunk_steps is not None and int(chunk_steps) < 1 or int(max_utterances) < 1:
        raise ValueError('chunk_steps and max_utterances are positive')
    mels = [torch.as_tensor(m) for m in mels]
    mels = [m.unsqueeze(0) if m.dim() == 2 else m for m in mels]
    if not mels or (seeds is not None and len(seeds) != len(mels)) or (global_rng and len(mels) != 1):
        raise ValueError('one seed per utterance, at least one utterance')
    device = next(model.parameters()).device
    if loop_fn is None:
        model._require_hip_device(device)
    mode, hop, C = model.mode, model.hop_length, model.n_classes
    mu_law = bool(mu_law) if mode == 'RAW' else False
    frames = [int(m.size(-1)) for m in mels]
    tail_len = 20 * hop
    for f in frames:               # the reference's tail fade raises here (:258), after its loop; this path before anything is launched
        if (f - 1) * hop < tail_len:
            raise ValueError(f'operands could not be broadcast together with shapes ({(f - 1) * hop},) ({tail_len},)')
    want32 = dtype == np.dtype(np.float32)
    was_training = model.training
    model.eval()
    loop_ms, n_slices, first_seen, warned = 0.0, 0, False, False
    slab_tuning = 8192 if getattr(model, 'slab_prep_split', False) else 0
    noise_bytes = int(getattr(model, 'noise_chunk_bytes', 2 << 30))
    try:
        with torch.no_grad():
            for utts in unbatched_groups(frames, int(max_utterances)):
                fr = [frames[u] for u in utts]
                plan = _unbatched_plan(fr, hop)
                n, T = len(utts), plan.T
                wave_len = np.array([(f - 1) * hop for f in fr], dtype=np.int32)
                seg_pos, seg_lim = plan.seg_pos, plan.seg_lim
                # the materialised conditioning of the group's utterances, concatenated (each starts on a frame boundary): score_corpus' pre-loop path
                if loop_fn is None and getattr(model, 'pre_algo', 'torch') == 'native':
                    pre = model._pre_engine()
                    mels_up = torch.empty(sum(fr) * hop, mels[utts[0]].size(1), dtype=torch.float32, device=device)
                    aux = torch.empty(sum(fr), 4 * model.aux_dims, dtype=torch.float32, device=device)
                    jobs = [(mels[u], mels_up[int(p):int(p) + f * hop], aux[int(p) // hop:int(p) // hop + f]) for u, p, f in zip(utts, seg_pos, fr)]
                    pre.upsample_many(jobs, rows=False, streams=int(getattr(model, 'pre_streams', 8)), batched=bool(getattr(model, 'pre_batched', True)))
                else:
                    ups, auxs = zip(*[model.conditioning(mels[u])[:2] for u in utts])
                    mels_up, aux = torch.cat(ups).contiguous(), torch.cat(auxs).contiguous()

                gens = {}

                def seed_streams():
                    """the reference's per-utterance CPU streams: one private generator per utterance, the GRUCell constructor draws burnt once"""
                    if noise_source != 'cpu':
                        return
                    for u in utts:
                        gens[u] = None if global_rng else torch.Generator(device='cpu').manual_seed(int(seeds[u]))
                        burn_ctor_draws(model.rnn_dims, model.aux_dims, 'cpu', gens[u])
                lib_ids = np.concatenate([library_seg_ids(seeds[u], 1) for u in utts]) if noise_source == 'library' else None
                lib_kw = dict(noise_seed=int(getattr(model, 'noise_key', 0)), noise_seg_id=lib_ids) if lib_ids is not None else {}

                def draw(s0, s1):
                    """noise rows of loop steps [s0, s1) of the group's segments, on the device (None: the loop draws them)"""
                    if noise_source == 'library':
                        if loop_fn is None:
                            return None
                        return torch.from_numpy(_lib.noise_fill_host(mode, n, C, s0, s1, lib_kw['noise_seed'], lib_ids)).to(device)
                    if noise_source != 'cpu':
                        return draw_steps(mode, n, s1 - s0, C, device, 'device')
                    per_utt = [draw_steps(mode, 1, s1 - s0, C, 'cpu', 'cpu', generator=gens[u]) for u in utts]
                    return pack_noise(mode, plan, per_utt, 0, n, steps=s1 - s0).to(device)

                def deliver(arr, t0, t1):
                    """chunks of steps [t0, t1) from arr [n][t1 - t0], in the group's order; copies, so that the staging buffer can be reused"""
                    nonlocal first_seen
                    for k, u in enumerate(utts):
                        if t0 < int(wave_len[k]):
                            if not first_seen and timings is not None:
                                timings['first_chunk_ms'] = (time.perf_counter() - t_call) * 1e3
                            first_seen = True
                            yield u, t0, arr[k, :min(t1, int(wave_len[k])) - t0].copy()

                if loop_fn is not None:         # the stand-in hook: the whole call at once, the chunks through wrnn_post_chunk_host
                    seed_streams()
                    segs = np.ascontiguousarray(torch.as_tensor(loop_fn(mels_up, aux, seg_pos, seg_lim, T, draw(0, T), hop)).cpu().numpy(), dtype=np.float32)
                    tail, lut = _post.chunk_host_tables(hop, C, mu_law)
                    k_steps = T if chunk_steps is None else min(int(chunk_steps), T)
                    for t0, t1 in [(a, min(T, a + k_steps)) for a in range(0, T, k_steps)]:
                        o64, o32 = _lib.post_chunk_host(segs, wave_len, t0, t1, tail, lut, want64=not want32, want32=want32)
                        n_slices += 1
                        yield from deliver(o32 if want32 else o64, t0, t1)
                    continue

                eng = model._loop_engine()
                kernel = eng.plan(n, T, algo=model.loop_algo)['kernel']
                resumable = kernel in RESUMABLE_KERNELS
                groups = model.loop_sparse_groups(eng, n, T) if hasattr(model, 'loop_sparse_groups') else 0
                sliced = chunk_steps is not None and resumable
                watched = bool(live) and chunk_steps is not None and kernel in WATCHABLE_KERNELS
                if chunk_steps is not None and not resumable and not watched and not warned:
                    import warnings
                    warnings.warn(_WARNED_WHOLE.format(kernel))
                    warned = True
                # the noise bound of generate() / generate_corpus: at most `model.noise_chunk_bytes` of it resident, on the kernels that continue a call
                bound = T
                if noise_source != 'library' and resumable:
                    bound = max(1, min(T, noise_bytes // (n * (11 if mode == 'MOL' else C) * 4)))
                out = torch.empty(n, T, dtype=torch.float32, device=device)
                run_kw = dict(algo=model.loop_algo, check=False, out=out, sparse_groups=groups, tuning=slab_tuning, **lib_kw)
                rng_state = torch.get_rng_state() if (global_rng and noise_source == 'cpu') else None

                def run(s0, s1):
                    eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, draw(s0, s1), hop, t_range=None if (s0 == 0 and s1 == T) else (s0, s1), **run_kw)

                seed_streams()
                if watched:
                    # ---- live: the WHOLE call is queued on the main stream and publishes how far it has got (wrnn_generate_segments_watched); ONE side
                    #      stream looks at the progress words and finishes and copies out every chunk the kernel has passed (these kernels leave most of
                    #      the chip idle: wrnn_post_chunk has CUs to run on beside them).  Every reader is launched AFTER the look that released its chunk.
                    k_steps = min(int(chunk_steps), T)
                    every = min(64, k_steps)                       # a chunk is late by at most one publication
                    main = torch.cuda.current_stream(device)
                    # (a HIGH-PRIORITY stream: the runtime keeps the hardware queues of a priority class apart from the others', so a look never sits
                    # behind the loop kernel in the main stream's hardware queue -- an ordinary side stream may be given that very queue when the
                    # process has few of them, and every chunk then arrives at the end)
                    side = torch.cuda.Stream(device, priority=-1)
                    t_dtype = torch.float32 if want32 else torch.float64
                    words = torch.zeros(eng.watch_words(n, T, algo=model.loop_algo), dtype=torch.int32, device=device)
                    words_pin = torch.zeros(words.numel(), dtype=torch.int32, pin_memory=True)
                    dev_buf = [torch.empty(n * k_steps, dtype=t_dtype, device=device) for _ in range(2)]
                    pin_buf = [torch.empty(n * k_steps, dtype=t_dtype, pin_memory=True) for _ in range(2)]
                    wl_dev = torch.from_numpy(wave_len).to(device)
                    _post.chunk_tables_on_device(hop, C, mu_law, device)      # (made here, on the main stream, not by the first launch on the side stream)
                    for d in dev_buf + [out, words, wl_dev]:
                        d.record_stream(side)                      # (read on the side stream: a generator closed early frees them safely)
                    zeroed, looked, loop_done = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
                    copy_done = [torch.cuda.Event() for _ in range(2)]
                    zeroed.record(main)
                    side.wait_event(zeroed)                        # no look in front of the zeroed words (and the tables)
                    eng.run_segments(mels_up, aux, seg_pos, seg_lim, T, draw(0, T), hop, watch=(words, every), **run_kw)
                    loop_done.record(main)
                    slices = [(a, min(T, a + k_steps)) for a in range(0, T, k_steps)]
                    done = 0
                    while done < len(slices):                      # ends with loop_done: the poll is bounded by the kernel itself
                        if loop_done.query():
                            m = T
                        else:
                            with torch.cuda.stream(side):
                                words_pin.copy_(words, non_blocking=True)
                            looked.record(side)
                            looked.synchronize()
                            m = int(words_pin.min())
                        upto = live_release(slices, done, m)
                        if upto == done:
                            time.sleep(0.0005)
                            continue
                        pending = None
                        for i in range(done, upto):
                            b, (t0, t1) = i % 2, slices[i]
                            d = dev_buf[b][:n * (t1 - t0)]
                            with torch.cuda.stream(side):
                                _post.chunk_on_device(out, wl_dev, t0, t1, hop, C, mu_law, out64=None if want32 else d, out32=d if want32 else None,
                                                      min_wave_len=int(wave_len.min()))
                                pin_buf[b][:n * (t1 - t0)].copy_(d, non_blocking=True)
                            copy_done[b].record(side)
                            n_slices += 1
                            if pending is not None:                # (slice i is queued: now the host may wait for slice i - 1)
                                pb, p0, p1 = pending
                                copy_done[pb].synchronize()
                                yield from deliver(pin_buf[pb][:n * (p1 - p0)].numpy().reshape(n, p1 - p0), p0, p1)
                            pending = (b, t0, t1)
                        pb, p0, p1 = pending                       # nothing else is released yet: the last one goes out at once
                        copy_done[pb].synchronize()
                        yield from deliver(pin_buf[pb][:n * (p1 - p0)].numpy().reshape(n, p1 - p0), p0, p1)
                        done = upto
                    if check:
                        eng.status()
                    side.synchronize()
                    model.last_loop_ms, model.last_loop_kernel = eng.last_loop_ms(), eng.last_loop_kernel()
                    loop_ms += model.last_loop_ms
                    continue
                if not sliced:
                    try:
                        for s0, s1 in _cut(0, T, bound):
                            run(s0, s1)
                    except _lib.ResidencyError as e:
                        import warnings
                        warnings.warn(f'wavernn_amd: {e}; redoing the group unsliced on the next kernel')
                        if rng_state is not None:
                            torch.set_rng_state(rng_state)
                        seed_streams()
                        run(0, T)
                else:
                    # ---- streamed: behind every step slice one wrnn_post_chunk launch on the SAME stream (the persistent loop kernel holds every CU: a
                    #      kernel on another stream would only wait behind it), an event, and the chunk's copy into one of two page-locked buffers on ONE
                    #      side stream (the copy engine).  The next slice is queued BEFORE the host waits for that copy.
                    k_steps = min(int(chunk_steps), T)
                    main = torch.cuda.current_stream(device)
                    side = torch.cuda.Stream(device)
                    t_dtype = torch.float32 if want32 else torch.float64
                    dev_buf = [torch.empty(n * k_steps, dtype=t_dtype, device=device) for _ in range(2)]
                    for d in dev_buf:
                        d.record_stream(side)                      # (read by the copies on the side stream: a generator closed early frees them safely)
                    pin_buf = [torch.empty(n * k_steps, dtype=t_dtype, pin_memory=True) for _ in range(2)]
                    post_done = [torch.cuda.Event() for _ in range(2)]
                    copy_done = [torch.cuda.Event() for _ in range(2)]
                    wl_dev = torch.from_numpy(wave_len).to(device)
                    pending, fell_back = None, False
                    slices = [(a, min(T, a + k_steps)) for a in range(0, T, k_steps)]
                    for i, (t0, t1) in enumerate(slices):
                        b = i % 2
                        try:
                            for s0, s1 in _cut(t0, t1, bound):
                                run(s0, s1)
                        except _lib.ResidencyError as e:
                            if i:
                                raise
                            # the persistent grid was refused on the first slice (a continuation cannot change kernels): the group unsliced on the
                            # next kernel, from the start of every utterance's noise stream -- what generate() and generate_corpus do
                            import warnings
                            warnings.warn(f'wavernn_amd: {e}; redoing the group unsliced on the next kernel')
                            if rng_state is not None:
                                torch.set_rng_state(rng_state)
                            seed_streams()
                            run(0, T)
                            fell_back = True
                            break
                        if i >= 2:
                            main.wait_event(copy_done[b])          # the copy of slice i - 2 has left this device buffer
                        w = t1 - t0
                        d = dev_buf[b][:n * w]
                        _post.chunk_on_device(out, wl_dev, t0, t1, hop, C, mu_law, out64=None if want32 else d, out32=d if want32 else None,
                                              min_wave_len=int(wave_len.min()))
                        post_done[b].record(main)
                        side.wait_event(post_done[b])
                        with torch.cuda.stream(side):
                            pin_buf[b][:n * w].copy_(d, non_blocking=True)
                        copy_done[b].record(side)
                        n_slices += 1
                        if pending is not None:                    # (slice i is queued: now the host may wait for slice i - 1)
                            pb, p0, p1 = pending
                            copy_done[pb].synchronize()
                            yield from deliver(pin_buf[pb][:n * (p1 - p0)].numpy().reshape(n, p1 - p0), p0, p1)
                        pending = (b, t0, t1)
                    if not fell_back:
                        pb, p0, p1 = pending
                        copy_done[pb].synchronize()
                        if check:
                            eng.status()                           # after the last slice: no wrnn_status between slices (it synchronises)
                        yield from deliver(pin_buf[pb][:n * (p1 - p0)].numpy().reshape(n, p1 - p0), p0, p1)
                        side.synchronize()
                        model.last_loop_ms, model.last_loop_kernel = eng.last_loop_ms(), eng.last_loop_kernel()
                        loop_ms += model.last_loop_ms
                        continue
                # ---- the loop ran whole: ONE unfold launch finishes every utterance of the group; each is delivered as one chunk
                from .post import unfold_on_device
                wav, sl = unfold_on_device(out, list(range(n)), [1] * n, [int(w) for w in wave_len], 0, hop, C, mu_law, False)
                host = torch.empty(wav.shape, dtype=wav.dtype, pin_memory=True)
                host.copy_(wav, non_blocking=True)
                if check:
                    eng.status()
                torch.cuda.current_stream(device).synchronize()
                model.last_loop_ms, model.last_loop_kernel = eng.last_loop_ms(), eng.last_loop_kernel()
                loop_ms += model.last_loop_ms
                host = host.numpy()
                n_slices += 1
                for k, u in enumerate(utts):
                    if not first_seen and timings is not None:
                        timings['first_chunk_ms'] = (time.perf_counter() - t_call) * 1e3
                    first_seen = True
                    yield u, 0, host[sl[k][0]:sl[k][1]].astype(dtype)       # (float32: the double rounded to nearest, as wrnn_post_chunk's out32)
    finally:
        if timings is not None:
            timings['loop_ms'], timings['slices'] = loop_ms, n_slices
        if was_training:
            model.train()


def generate_unbatched(model, mels: Sequence, mu_law: bool, seeds: Optional[Sequence[int]] = None, noise_source='library', chunk_steps: Optional[int] = None,
                       on_chunk=None, max_utterances: int = 64, dtype=np.float64, loop_fn=None, check=True, timings: Optional[dict] = None, live=False):
    """Generate every utterance of `mels` (each (1, feat, N_u) or (feat, N_u)) UNBATCHED -- no folds, no cross-fade seams: the quality mode of
    `generate(batched=False)` -- as the unfolded segments of one loop call per group, and optionally hand the audio on in step slices while the loop
    goes on.  Returns the list of waveforms (`dtype`, (N_u - 1) * hop samples each) in the caller's order.

    Groups: the utterances sorted by frame count (stable, longest first) and cut into groups of at most `max_utterances`; a group is ONE segment
    table over the concatenated, materialised conditioning (seg_pos = o_u, seg_lim = o_u + N_u * hop, T = the group's longest N_u * hop), so a list
    costs its longest utterance, not the sum.  The default of 64 is where the dense latency kernel's step time is still flat (wrnn_chain_kernel
    carries 4 clusters x 16 segments at the step time of one); a pruned model (wrnn_sparse_kernel) may be given 256.

    Noise: 'library' (default): utterance u under the stream id `library_seg_ids(seeds[u], 1)` and the key `model.noise_key` -- its audio equals
    `generate(mel_u, ..., batched=False, ...)` alone with `model.noise_source = 'library'` and `model.noise_seed = seeds[u]`.  'cpu': one private
    generator per utterance seeded seeds[u], the constructor draws burnt once, drawn in step slices bounded by `model.noise_chunk_bytes` -- the
    reference's unbatched `generate` after `torch.manual_seed(seeds[u])`.  'device': the device generator (`seeds` unused).

    chunk_steps=None: the loop runs whole (or in noise slices) and `wrnn_post_unfold` finishes all utterances of a group in one launch.
    chunk_steps=k, on a kernel that continues a call (`engine.RESUMABLE_KERNELS`): the loop runs in slices of k steps; behind every slice one
    `wrnn_post_chunk` launch on the same stream and the chunk's copy into one of two page-locked buffers on a side stream, the next slice queued
    before the host waits for that copy.  Any other kernel runs the call whole and delivers each utterance as one chunk at the end (one warning).
    live=True with chunk_steps=k, on a kernel that is launched once for all steps (`engine.WATCHABLE_KERNELS`: every model of non-shipped dims): the
    call is queued whole and publishes its progress every min(64, k) steps (`wrnn_generate_segments_watched`); one side stream looks at the progress
    words about every 0.5 ms and runs `wrnn_post_chunk` and the chunk's copy for every slice of k steps the kernel has passed, while it goes on --
    the same chunks, in the same order, with the same bits as the sliced path would deliver.  On a kernel that continues a call `live` changes
    nothing (the sliced path), nor on wrnn_stream_kernel (whole, with the warning), nor under `loop_fn`.

    on_chunk(u, start, samples), on the calling thread, in step order and within a slice in the group's order, for every utterance with
    start < wave_len_u: `samples` (length min(t1, wave_len_u) - start) is a copy the callee may keep.  The returned waveforms are assembled from
    the same chunks.  check=True: `eng.status()` after the last slice of a group (never between slices: it synchronises); raises if a kernel gave up.
    A mel of fewer than 21 frames raises the reference's ValueError (wave_len < 20 * hop, :258) before anything is launched.

    loop_fn: the stand-in hook of `generate_corpus`, same signature; the chunks then go through `wrnn_post_chunk_host`, so the whole host path runs
    without a GPU.  timings: optional dict, receives loop_ms (summed over the groups), first_chunk_ms (wall time from the call to the first chunk)
    and slices (post-loop launches)."""
    parts = [[] for _ in mels]
    for u, start, samples in unbatched_chunks(model, mels, mu_law, seeds=seeds, noise_source=noise_source, chunk_steps=chunk_steps,
                                              max_utterances=max_utterances, dtype=dtype, loop_fn=loop_fn, check=check, timings=timings, live=live):
        assert start == sum(len(p) for p in parts[u])
        if on_chunk is not None:
            on_chunk(u, start, samples)
        parts[u].append(samples)
    return [p[0] if len(p) == 1 else np.concatenate(p) for p in parts]
