/*
 * wavernn_amd.h -- C ABI of the MI355X-native WaveRNN generate path (libwavernn_amd.so).
 *
 * Drop-in boundary for ONE hot path of fatchord/WaveRNN: the per-sample loop of
 * `WaveRNN.generate()` (reference models/fatchord_version.py:169-264).  The reference has no FFI of its
 * own (it is pure Python on PyTorch); these entry points are what a binding for that path binds, one per
 * reference stage, and each cites the reference lines it replaces.  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every `const float*` marked "device" is a HIP device pointer owned by the caller
 *     (e.g. a torch tensor's data_ptr()); the library BORROWS it for the duration of the call.
 *   - all functions return WRNN_OK (0) or a negative error code; wrnn_last_error() returns a message for the
 *     calling thread's last failure.  Nothing here synchronises the device except the functions that say so.
 *   - a wrnn_pack is immutable after creation: any number of threads / streams may generate from one pack at the same
 *     time, each with its own workspace (and timer).  Nothing is read from the environment.
 *   - work is enqueued on the hipStream_t passed as `void* stream` (NULL = default stream).
 *   - arithmetic type: float32 (same as the reference).  No CPU fallback exists: without a HIP device every
 *     compute entry point fails with WRNN_ERR_NO_DEVICE.
 */
#ifndef WAVERNN_AMD_H
#define WAVERNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WRNN_ABI_VERSION 9   /* v9 + wrnn_nll, wrnn_nll_host (appended like wrnn_noise_fill: the number stays, the symbols tell whether a library has them): the loss of a teacher-forced call.  v9 + wrnn_options.noise_lib / noise_seed / noise_seg_id, wrnn_noise_fill, wrnn_noise_fill_host (appended like sparse_groups: the number stays): the sampling noise drawn inside the library.  v9 + wrnn_options.sparse_groups (appended; struct_bytes tells whether a caller has it: the number stays, every v9 caller runs as it did): two groups per cluster of wrnn_sparse_kernel, on request.  v9 (round 6): wrnn_pack_sparse_fc_blocks -- block-sparse Linear layers in wrnn_sparse_kernel.  v8 (round 6): WRNN_ALGO_OCTO (wrnn_octo_kernel: one 512-thread workgroup per CU, matrix waves + service waves; dense MOL).  v7 (round 5): WRNN_ALGO_CHAIN (wrnn_chain_kernel, what `auto` runs for <= 128 segments of a dense model, MOL or 9-bit RAW); WRNN_ALGO_SPARSE is the rebuilt wrnn_sparse_kernel (slabbed, resumable, takes mel_stage) and what `auto` picks for a qualifying pack; wrnn_options.depth does not apply to it.  v6 (round 4): wrnn_options.mel_stage & co + wrnn_pre_upsample_rows -- the last up-sampling stage formed inside wrnn_duo_kernel.  v5 (round 4): WRNN_ALGO_DUO runs RAW too; `auto` never degrades inside the library (WRNN_ERR_RESIDENCY: the caller re-plans); tuning bits per kernel */

enum {
    WRNN_OK = 0,
    WRNN_ERR_ARG = -1,        /* bad argument (shape, NULL pointer, unsupported dims) */
    WRNN_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime failure */
    WRNN_ERR_HIP = -3,        /* a HIP API call failed; see wrnn_last_error() */
    WRNN_ERR_WORKSPACE = -4,  /* workspace too small */
    WRNN_ERR_KERNEL = -5,     /* a kernel reported a failure (bounded spin expired, bad state) */
    WRNN_ERR_RESIDENCY = -6   /* persistent grid cannot be co-resident on this device */
};

enum { WRNN_MODE_RAW = 0, WRNN_MODE_MOL = 1 };  /* reference: WaveRNN(mode='RAW'|'MOL'), fatchord_version.py:97-104 */

/* Loop kernel selection. */
enum {
    WRNN_ALGO_AUTO = 0,     /* shipped dims, MOL or RAW with 512 classes: WRNN_ALGO_SPARSE when a MOL pack qualifies (wrnn_pack_sparse_blocks() > 0) on a
                               device of >= 256 CUs (a qualifying 9-bit RAW pack keeps the dense kernels: WRNN_ALGO_SPARSE runs it on request), else
                               WRNN_ALGO_CHAIN (<= 128 segments, >= 256 CUs), else WRNN_ALGO_DUO (>= 256 CUs: always its 4 clusters), else
                               WRNN_ALGO_LOOP (>= 64 CUs: 1 or 2 clusters; also when wrnn_options.clusters asks `auto` for fewer than 4), else -- and for
                               RAW with fewer classes -- WRNN_ALGO_STREAM; other dims, and RAW with more classes: wrnn_generic_kernel.  The planner's one table of the
                               kernels: KINDS in csrc/wrnn_abi.hip */
    WRNN_ALGO_STREAM = 1,   /* one workgroup per folded segment, weights streamed from L2/MALL each step: the generic fallback
                               (any class count, any device size) and the on-GPU cross-check */
    WRNN_ALGO_LOOP = 2,     /* role-split pipelined persistent kernel (RAW and MOL): up to 4 clusters of 64 CUs, each with a full
                               fp32 copy of the loop weights in registers, up to 8 groups of <= 16 segments in flight per cluster,
                               tag-free activation exchange in MFMA-fragment order (csrc/wrnn_loop.hip) */
    WRNN_ALGO_DUO = 6,      /* the loop kernel cut for TWO workgroups per CU (MOL and RAW): four roles -- rnn1 / rnn2 x {W_ih + fc, W_hh [+ fc3 and
                               sampling]} -- of <= 128 weight registers, 128 workgroups per 64-CU cluster, so that one wave's MFMAs overlap
                               the other's loads, pointwise math and barrier waits (csrc/wrnn_duo.hip); >= 64 CUs.  What `auto` runs for a dense pack
                               beyond 128 segments on >= 256 CUs */
    WRNN_ALGO_CHAIN = 7,    /* the single-stream latency kernel (MOL and 9-bit RAW, >= 256 CUs): one workgroup per CU, <= 4 groups of <= 16 segments in flight per
                               64-CU cluster (256 segments a round; more: further rounds), both halves of a GRU cell's rows in one workgroup (gh never leaves the registers), rnn2 + fc1 + fc2
                               on one XCD (csrc/wrnn_chain.hip).  What `auto` runs for one utterance (<= 128 segments) of a dense model */
    WRNN_ALGO_OCTO = 8,     /* the WAVE-SPECIALISED form of the dense loop kernel (MOL, >= 256 CUs, on request only; round 6): ONE 512-thread workgroup per CU -- four matrix
                               waves (W_ih and W_hh of the CU's 16 units in registers, the fc tile in LDS: operand by LDS-DMA, MFMA block, partial tiles)
                               and four service waves (partial sums, GRU cell, publishes, conditioning, fc3 + sampling) that meet through LDS counters;
                               gh never leaves the CU.  Same split, workspace, exchange buffer and state layout as WRNN_ALGO_DUO (csrc/wrnn_octo.hip) */
    WRNN_ALGO_TILE = 10,    /* wrnn_generic_kernel's dataflow for a TILE of up to 16 segments per workgroup (csrc/wrnn_tile.hip; on request only, `auto` never
                               picks it): generic packs only -- non-shipped dims, or RAW with more than 512 classes --, the pack as it is; ceil(n_segments / 16)
                               workgroups that never wait for one another, every matrix product on v_mfma_f32_16x16x4_f32 with the 16 segments as its N, so the
                               weights are streamed once per 16 segments and step.  Whole calls only (no step range), no mel_stage, no sparse_groups; workspace,
                               noise_lib, progress, timer and info as on wrnn_generic_kernel.  THE LDS RULE: the activations of the 16 segments live in LDS,
                               16 * 4 * (up4(1 + feat + aux) + 2 * up4(max(rnn, fc) + aux) + 2 * up4(rnn)) + 2560 bytes (up4: rounded up to a multiple of 4),
                               and must fit one CU's 160 KiB = 163840 (rnn = fc = 512, feat 80, aux 32: 145152; rnn = fc = 576 still fits, 640 does not); RAW: <= 2048
                               classes.  Other dims: WRNN_ERR_ARG with the bytes needed -- stay on `auto`.
                               THE WIDE FORM (csrc/wrnn_tile_wide.hip, wrnn_tile_wide_kernel): wrnn_options.clusters = 2, 4 or 8 spreads the rows of every
                               matrix stage of a tile over that many workgroups, which hand the stage's output to one another through the workspace (one
                               all-gather per stage); the samples and logits are wrnn_tile_kernel's bit for bit.  ONE round: ceil(n_segments / 16) * clusters
                               workgroups, at most one per CU, launched cooperatively -- more segments than that: WRNN_ERR_ARG (the text names the largest
                               count), a refused launch: WRNN_ERR_RESIDENCY; plain tile runs either call.  Every refusal and option of tile applies; the
                               workspace grows by the hand-off buffers (by tiles and dims, not by T); a kernel that gives up waiting: wrnn_status() */
    WRNN_ALGO_TILE_SPARSE = 12, /* WRNN_ALGO_TILE for a PRUNED model of non-shipped dims (csrc/wrnn_tile_sparse.hip, wrnn_tile_sparse_kernel; on request only): the
                               same dataflow, LDS rule, workspace and options, but the four GRU matrices -- and fc1 / fc2 -- run as gathered block-sparse MFMA
                               stages over the pack's TILE-SPARSE VIEW, so the pruned 16x1 blocks are neither streamed nor multiplied.  wrnn_pack_create builds
                               the view for a generic pack (wrnn_pack_tile_sparse()): a block row is 16 consecutive rows of one gate (GRU: 3 gates, Linear: 1), a
                               block (block row, column -- over the whole K, aux columns included) survives if any of its 16 values is non-zero; the GRU view
                               exists when rnn % 16 == 0 and AT MOST 41 % of the blocks of each of rnn1 / rnn2 weight_ih / weight_hh survive, the fc view in
                               addition when fc % 16 == 0 and the same holds for fc1 and fc2.  (41 %: a model block-pruned to 60 % sparsity -- 40.01 % survive the
                               per-gate rounding -- is the least sparse one at which the kernel measured no slower than WRNN_ALGO_TILE, profiles/tile_sparse_ab.json;
                               at one half it ran at 0.87 x.)  Without a view: WRNN_ERR_ARG naming the matrix and its surviving
                               fraction, or the dim -- WRNN_ALGO_TILE runs such a pack dense.  An output element is one accumulator chain over its block row's
                               surviving columns in ascending order */
    WRNN_ALGO_TILE_BF16 = 13, /* WRNN_ALGO_TILE with the weights in BFLOAT16 (csrc/wrnn_tile_bf16.hip, wrnn_tile_bf16_kernel; on request only, `auto` never picks
                               it).  NOT THE REFERENCE'S ARITHMETIC: the eight loop matrices (I, rnn1 / rnn2 weight_ih / weight_hh, fc1, fc2, fc3) are rounded
                               once, when the pack is built, to bfloat16, round-to-nearest-even; biases, activations, the GRU state and every pointwise pass
                               stay float32.  THE ARITHMETIC CONTRACT: where an activation x is multiplied it is split in registers into three bf16 pieces by
                               truncation -- hi = x & 0xFFFF0000, mid = (x - hi) & 0xFFFF0000, lo = x - hi - mid; hi + mid + lo == x exactly -- and the three
                               products run on v_mfma_f32_16x16x32_bf16 into ONE float32 accumulator per output element, k-steps of 32 ascending, hi / mid /
                               lo inside a step (the r and z gates of a GRU: W_ih's k-steps, then W_hh's, in one chain): float32 sums of exact products on
                               the ROUNDED weights, i.e. what WRNN_ALGO_TILE computes on a model whose eight matrices were rounded the same way
                               (wavernn_amd.synthetic.bf16_round_state_dict), up to the summation order.  What the rounding costs a checkpoint, in bits per
                               sample: score it with WRNN_ALGO_TILE_BF16 and with WRNN_ALGO_TILE (score_wavernn --algo).  Same dataflow, grid, workspace,
                               options and refusals as WRNN_ALGO_TILE, and THE SAME LDS RULE (row counts rounded up to 4; rnn = fc = 512 and 576 at feat 80,
                               aux 32 fit, 640 does not); RAW: <= 2048 classes.  wrnn_pack_create builds the bf16 view for every generic pack whose dims
                               pass that rule (wrnn_pack_tile_bf16()) unless a weight is not finite or rounds to +-inf; without a view: WRNN_ERR_ARG.
                               Measured against WRNN_ALGO_TILE on the same pack, T = 2000 (profiles/tile_bf16_ab.json): 1.76 - 1.81 x its throughput at 64 - 1024
                               segments of a MoL model with rnn = fc = 256 (93 -> 52 us per step), 1.71 - 1.72 x for 10-bit RAW at 512 (306 -> 178), 2.03 - 2.05 x
                               for MoL at 576 (417 -> 205) */
    WRNN_ALGO_SPARSE = 5    /* block-sparse GRU kernel (MOL, BASELINE config 5; or 9-bit RAW = 512 classes -- fc3 a dense stage of every workgroup,
                               four sampling workgroups per cluster): needs GRU matrices whose 16x1 block rows keep <= 64 columns
                               (wrnn_pack_sparse_blocks) and >= 256 CUs; fc1 / fc2 are gathered too when they are block-sparse (wrnn_pack_sparse_fc_blocks); 16 clusters of 16 CUs, ONE group of <= 16 segments each: a
                               step is the latency of one chain, sixteen chains run side by side (csrc/wrnn_sparse.hip).  wrnn_options.sparse_groups = 2: TWO groups
                               per cluster, stage by stage through the same weights (MOL with block-sparse Linear layers; 512 segments a round) */
};

/*
 * Host-side view of the loop weights, exactly the tensors `WaveRNN.generate()` touches inside its loop
 * (state_dict keys in comments; shapes for rnn_dims=H, fc_dims=F, feat_dims=M, aux_dims=A=res_out_dims/4,
 * n_classes=C).  fatchord_version.py:115-123 (definition), :208-223 (use), :273-279 (GRU cell views).
 * All pointers are HOST pointers to contiguous row-major float32.
 */
typedef struct wrnn_weights {
    int32_t rnn_dims;    /* H: 512 for the MFMA kernels (loop / duo / sparse / stream); any other value <= 2048 runs on wrnn_generic_kernel */
    int32_t fc_dims;     /* F: 512 for the MFMA kernels; <= 2048 otherwise */
    int32_t feat_dims;   /* M: 80 for the MFMA kernels; feat + aux <= 1024 otherwise */
    int32_t aux_dims;    /* A: 32 for the MFMA kernels */
    int32_t n_classes;   /* C: 30 (MOL) or 2**bits (RAW), 2..2048; shipped dims: the loop kernels need 512, 2..511 stream, 513..2048 run on
                            wrnn_generic_kernel like non-shipped dims */
    int32_t mode;        /* WRNN_MODE_* */
    const float *I_w, *I_b;                          /* I.weight (H,1+M+A), I.bias (H) */
    const float *w_ih1, *w_hh1, *b_ih1, *b_hh1;      /* rnn1.weight_ih_l0 (3H,H), weight_hh_l0 (3H,H), biases (3H) */
    const float *w_ih2, *w_hh2, *b_ih2, *b_hh2;      /* rnn2.weight_ih_l0 (3H,H+A), weight_hh_l0 (3H,H), biases (3H) */
    const float *fc1_w, *fc1_b;                      /* fc1.weight (F,H+A), fc1.bias (F) */
    const float *fc2_w, *fc2_b;                      /* fc2.weight (F,F+A), fc2.bias (F) */
    const float *fc3_w, *fc3_b;                      /* fc3.weight (C,F), fc3.bias (C) */
} wrnn_weights;

/* Opaque device-resident weight pack (replaces the per-call `get_gru_cell` views, fatchord_version.py:178-179). */
typedef struct wrnn_pack wrnn_pack;

/*
 * Geometry of one batched (folded) or unbatched generation -- the arguments of
 * `fold_with_overlap(x, target, overlap)` (fatchord_version.py:293-340) without materialising the fold:
 * segment b, step t reads the un-folded conditioning at position p = b*stride + t; positions p >= L are the
 * reference's zero padding (:326-330).  Unbatched: B=1, T=L, stride=0.
 */
typedef struct wrnn_geometry {
    int32_t B;        /* number of folded segments (num_folds) */
    int32_t T;        /* steps per segment: target + 2*overlap (batched) or L (unbatched) */
    int32_t stride;   /* target + overlap */
    int32_t L;        /* un-folded conditioning length in samples (N*hop) */
    int32_t hop;      /* samples per mel frame (aux is constant over a frame: Stretch2d, :57-61,:84) */
    int32_t n_frames; /* rows of `aux` (= L / hop) */
} wrnn_geometry;

/* HIP-event timer owned by the CALLER (one per in-flight call): wrnn_generate* records an event pair around every loop-kernel
 * launch it enqueues.  Keeps the weight pack immutable, so one pack can serve several streams / threads at once. */
typedef struct wrnn_timer wrnn_timer;

/* What a wrnn_generate* call decided (filled synchronously, before the call returns). */
typedef struct wrnn_run_info {
    const char *kernel;      /* "wrnn_duo_kernel" / "wrnn_octo_kernel" / "wrnn_chain_kernel" / "wrnn_sparse_kernel" / "wrnn_loop_kernel" / "wrnn_stream_kernel" / "wrnn_generic_kernel" / "wrnn_tile_kernel" /
                                "wrnn_tile_sparse_kernel" / "wrnn_tile_bf16_kernel" / "wrnn_tile_wide_kernel" */
    int32_t units_per_wg;    /* hidden units per workgroup (16; sparse: 64; stream: 0) */
    int32_t clusters;        /* independent CU clusters, each holding one copy of the weights; wrnn_tile_wide_kernel: workgroups per tile of 16 segments (2, 4, 8),
                                with units_per_wg = 16, depth = 0, rounds = 1, launches = 1, slab_steps = T */
    int32_t depth;           /* groups of <= 16 segments in flight per cluster */
    int32_t rounds;          /* rounds of clusters x depth groups the segments were cut into */
    int32_t slab_steps;      /* steps per launch of a persistent kernel = one conditioning slab (wrnn_loop_kernel: steps of hoisted cI
                                materialised at a time; duo / sparse: steps one set of per-segment aux tables covers).  wrnn_plan_segments()
                                does not know the hop: there this is an UPPER BOUND -- a duo / sparse call caps it at 6 hops + 1 steps */
    int32_t launches;        /* loop-kernel launches enqueued */
} wrnn_run_info;

/*
 * Per-call options (replaces the environment variables ABI v2 read at call time).  Zero-initialise, set struct_bytes =
 * sizeof(wrnn_options); NULL options = all defaults.  Everything here is read during the call only.
 */
typedef struct wrnn_options {
    int32_t struct_bytes;
    int32_t algo;            /* WRNN_ALGO_*                                                                  (default AUTO) */
    int32_t depth;           /* groups in flight per cluster, 1..8 (sparse: does not apply -- see sparse_groups); 0 = the library picks */
    int32_t clusters;        /* loop kernel: clusters to use (1, 2 or 4); 0 = the library picks.  WRNN_ALGO_TILE: workgroups per tile -- 0 or 1 = wrnn_tile_kernel,
                                2, 4, 8 = wrnn_tile_wide_kernel, anything else WRNN_ERR_ARG; WRNN_ALGO_TILE_SPARSE / _TILE_BF16: a value above 1 is WRNN_ERR_ARG */
    int32_t cond_valu;       /* stream kernel: 1 = hoisted conditioning on VALU instead of MFMA (cross-check) */
    int32_t slab_steps;      /* loop kernel: conditioning slab length in steps; 0 = sized to ~96 MB */
    int32_t t_begin, t_end;  /* run steps [t_begin, t_end) of the T; 0,0 = all.  t_begin > 0 CONTINUES the call that ended at
                                t_begin on the same workspace (wrnn_loop / _duo / _sparse / _chain_kernel); `noise` then covers [t_begin, t_end) only,
                                `out` / force_x / logits always the whole [.., T] tensors */
    int32_t tuning;          /* A/B switches for measurements, PER KERNEL (0 = the measured defaults; results never depend on them):
                                wrnn_loop_kernel: bit 0 = no one-stage look-ahead of the exchange loads, bit 1 = full __syncthreads() fences
                                  at the stage barriers, bit 2 = no fused stages, bit 3 = RAW sampled by role A alone, bit 4 = RAW: one
                                  sampling workgroup per slot, bit 5 / bit 6 = never / always start a stage with the pending back half
                                  (default: up to 2 groups in flight), bit 7 = library exp / tanh in the MoL gate math;
                                wrnn_duo_kernel: bit 0 = the ih workgroups load a stage's operand into registers BEHIND the pending back half, bit 9 = in front
                                  of it (default: from 4 groups in flight), bit 1 = they fetch it into LDS one stage ahead (on request only), bit 2 = re-fill
                                  the exchange ring with the sentinel before EVERY launch, bit 3 = no second request for x_{t-1}, bit 4 = a fresh y2 request
                                  at the top of the sampling stage, bit 5 = sampling stage at wave priority 0, bit 7 = the residual input word requested beside
                                  the operand loads (round 5), bit 20 = the hh workgroups' gh block as ONE unbroken MFMA stream (bits 21-25: yield length /
                                  spacing of the broken one), bit 6 = placement read-out through phase_clocks (test hook), bit 12 = the polling stages check all 32 operand words of a lane for the
                                  sentinel instead of one word per 16-byte fragment (round 7; not in the phase-clock builds), bit 8 = every layer written
                                  through (no XCD-local plain stores), bit 14 = with phase_clocks: the stage time line of three steps as well
                                  (phase_clocks then holds [256 * 32 + 512 * 512] words; scripts/gpu_duo_trace.py);
                                wrnn_duo / _chain / _sparse_kernel (read by the library, by no kernel): bit 13 = a slab's derived MoL noise, its aux tables and the clearing
                                  of the placement words by three calls (two launches and a memset) instead of the one wrnn_slab_prep_kernel launch;
                                wrnn_sparse_kernel, wrnn_chain_kernel: bits 2, 8 as wrnn_duo_kernel; wrnn_sparse_kernel: bit 11 = the DENSE fc stages on a pack whose
                                  Linear layers are block-sparse too, bit 4 = MOL with gathered fc stages: y2 published and fc3 run densely by the sampling
                                  workgroup instead of folded into the fc2 tiles (RAW: no effect -- y2 is always published); wrnn_chain_kernel: bit 5 = MoL's fc3 tiles read from LDS (round 5).
                                When the two-workgroups-per-CU grid of wrnn_duo_kernel is refused the call returns WRNN_ERR_RESIDENCY; the
                                caller may run it again with WRNN_ALGO_LOOP (another workspace layout: query its size) or _STREAM. */
    const float *force_x;    /* device [n,T]: value fed back as x_t instead of the sample (teacher forcing): the waveform a scoring call walks
                                (wrnn_nll's `target`), and what the parity tests feed to compare logits step by step */
    float *logits;           /* device [T,n,C]: fc3 output of every step (:223) -- with force_x the output of the reference's teacher-forced
                                `WaveRNN.forward` (:131-167), what wrnn_nll scores; also read by the parity tests */
    unsigned long long *phase_clocks; /* profiling hook, device [256 workgroups][32] zeroed by the caller: wrnn_loop_kernel (MOL and RAW) and
                                wrnn_duo_kernel (MOL) add their per-(phase, stage segment) shader clocks (layouts: csrc/wrnn_loop.hip,
                                csrc/wrnn_duo.hip, "PROF"); with tuning bit 6: the placement read-out of wrnn_duo / _sparse_kernel instead */
    wrnn_timer *timer;       /* optional: time the loop kernel(s) of this call */
    wrnn_run_info *info;     /* optional out */
    /* optional progress read-out (ABI v4) -- the reference's `gen_display` (fatchord_version.py:241, :267-271: a rate line every
     * 100 steps of its Python loop).  Here the loop is one persistent kernel per conditioning slab, so the read-out exists per
     * slab: after the launches of every slab a host function is enqueued on `stream` (hipLaunchHostFunc) that calls
     * progress(steps_done, T, n_segments, progress_user) from a HIP runtime thread once the device has really got there.  No
     * synchronisation, nothing inside the kernel.  The callback must not call into HIP.  Loop kernel only (the other kernels are
     * one launch: they report once, at the end). */
    void (*progress)(int32_t steps_done, int32_t T, int32_t n_segments, void *user);
    void *progress_user;
    /* the LAST up-sampling stage inside the loop (ABI v6; wrnn_duo_kernel, wrnn_sparse_kernel, wrnn_chain_kernel -- any other kernel: WRNN_ERR_ARG).  The reference
     * up-samples the mel in three Stretch2d + box-conv stages and crops `indent` samples off both ends (fatchord_version.py:73-80,
     * :86-88) before the loop reads one [M] row per sample.  With mel_stage = 1 the `mels_up` argument of wrnn_generate* is the INPUT of
     * the last of those stages instead -- [mel_rows][M], what wrnn_pre_upsample_rows() writes: 1 / mel_scale of the rows -- and the loop
     * forms the row of step t of segment b from the three input rows its 2 * mel_scale + 1 taps reach, at the un-cropped position
     * j = seg_pos[b] + t + seg_moff[b] (one utterance: seg_moff = indent = pad * hop; utterance u of a concatenation whose S2 blocks
     * follow one another: indent * (2 u + 1)).  seg_pos / seg_lim / L / aux keep their meaning (the cropped time line).
     * This build: mel_scale == 11. */
    int32_t mel_stage;       /* 0 = `mels_up` is the up-sampled mel [L, M] (default) */
    int32_t mel_rows;        /* rows of `mels_up` when mel_stage = 1 */
    int32_t mel_scale;       /* stretch factor of the last stage */
    const float *mel_taps;   /* HOST [2 * mel_scale + 1]: upsample.up_layers.5.weight */
    const int32_t *seg_moff; /* HOST [n_segments] */
    /* wrnn_sparse_kernel, on request (`auto` never sets it): groups of <= 16 segments per 16-CU cluster.  0 or 1 = one (the default: every plan, workspace
     * size and output is what it was); 2 = two -- a round takes 32 groups (512 segments): groups 0-15 are the first slot of clusters 0-15, groups 16-31 the
     * second, and every stage of a step runs for the first slot and then for the second, so that one slot's exchange hops pass under the other's work.  A
     * segment's samples do not depend on it (same arithmetic, same order).  wrnn_run_info then reports depth = 2 and rounds = ceil(groups / 32); state, ring
     * and aux tables are sized for it by wrnn_workspace_bytes*.  Built for MOL packs whose Linear layers are block-sparse too (wrnn_pack_sparse_fc_blocks()
     * > 0).  WRNN_ERR_ARG: any other value; 2 on a call that does not run wrnn_sparse_kernel, on 9-bit RAW, on dense Linear layers (also tuning bit 11), or
     * with phase_clocks.  A caller whose struct_bytes ends before this field gets 0.  wrnn_abi_version() does NOT tell whether a library knows the field (it
     * stays 9): a library built before it reads only its own shorter struct and silently runs one group -- ask wrnn_plan_segments() and look at depth. */
    int32_t sparse_groups;
    /* The sampling noise drawn INSIDE the library from a counter-based generator (Philox4x32-10, csrc/wrnn_philox.h) instead of read from `noise`.
     * 0 (default): every plan, workspace size and output is what it was.  1: the `noise` argument of wrnn_generate* must be NULL (a pointer is
     * WRNN_ERR_ARG: no caller may believe their tensor was used); for every conditioning slab the library fills that slab's noise into the workspace, on the
     * stream, in front of the slab's loop launches -- the values wrnn_noise_fill() writes for the same (seed, ids, steps), so the samples are those of the
     * same call fed that tensor.  The value of (segment b, step t, index j) depends on noise_seed, the segment's id, t and j alone: not on the batch the
     * segment runs in, its position in it, the slab length, the step range of a continued call or the kernel.  The workspace grows by one slab of noise:
     * MOL 11 * n_segments floats per step, RAW n_classes * n_segments (the one-launch kernels wrnn_stream_kernel / wrnn_generic_kernel: all T steps; RAW on a
     * kernel that forms its conditioning in the loop: the default slab is what holds 2 GB of noise, at most 4096 steps, instead of 4096).  WRNN_ERR_ARG: any
     * other value.  A caller whose struct_bytes ends before these fields gets 0; as with sparse_groups, wrnn_abi_version() does not tell whether a library knows
     * them -- the symbol wrnn_noise_fill does. */
    int32_t noise_lib;
    uint64_t noise_seed;           /* the Philox key of the call */
    const uint64_t *noise_seg_id;  /* HOST [n_segments]: the 64-bit stream id of every segment; NULL: segment b has id b */
} wrnn_options;

const char *wrnn_last_error(void);
int wrnn_abi_version(void);

/* Number of compute units of HIP device `device` (or <0). */
int wrnn_device_cus(int device);

/* Upload + re-layout the loop weights for `device`.  Synchronous (uses its own stream and waits). */
int wrnn_pack_create(const wrnn_weights *w, int device, wrnn_pack **out);
void wrnn_pack_destroy(wrnn_pack *p);
/* bytes of loop weights the reference streams per step (the W of SURVEY.md section 8d) */
size_t wrnn_pack_weight_bytes(const wrnn_pack *p);
/* block sparsity of the pack's GRU matrices: the largest number of non-zero 16x1 blocks in any (matrix, gate, 16-row) block
 * row -- positive when WRNN_ALGO_SPARSE can run this pack (<= 64; MOL, or RAW with 512 classes), negated when it cannot */
int wrnn_pack_sparse_blocks(const wrnn_pack *p);
/* (v9) the same figure for fc1 / fc2 (their first H columns; 32 block rows of 16 each): positive when the Linear layers are block-sparse
 * too -- the reference's pruning recipe prunes them with the GRUs, notebooks/"Pruning - Scratchpad.ipynb":199-204 -- and
 * wrnn_sparse_kernel runs its GATHERED fc stages (no dense fc1 / fc2 MFMA blocks on the chain); negated: dense fc stages */
int wrnn_pack_sparse_fc_blocks(const wrnn_pack *p);
/* The tile-sparse view of a generic pack (WRNN_ALGO_TILE_SPARSE): 0 none (and every pack of the shipped dims), 1 the four GRU matrices, 2 fc1 / fc2 too.
 * kept / total (either may be NULL): surviving and all 16x1 blocks of rnn1.weight_ih, rnn1.weight_hh, rnn2.weight_ih, rnn2.weight_hh, fc1.weight, fc2.weight
 * (0 / 0 where the matrix's rows per gate are no multiple of 16: nothing was counted). */
int wrnn_pack_tile_sparse(const wrnn_pack *p, int32_t kept[6], int32_t total[6]);
/* The bf16 view of a generic pack (WRNN_ALGO_TILE_BF16): its bytes, 0 for none -- a pack of the shipped dims, dims past the LDS rule, or a weight that is
 * not finite or rounds to +-inf in bfloat16 (wrnn_pack_create still succeeds, and wrnn_last_error() names the matrix). */
size_t wrnn_pack_tile_bf16(const wrnn_pack *p);
/* Test hook, host only (no device, the HIP runtime is not touched): the packing routine of the bf16 view on ONE row-major matrix W [rows][K].  Returns the
 * number of bf16 elements of the image (or WRNN_ERR_ARG: a value is not finite or rounds to +-inf) and, when `out` is non-NULL and the image fits `cap`
 * elements, fills
 *   out  [ceil(K / 32)][rows][4 kq][8 j]   W[row][32 s + 4 j + kq] rounded to bfloat16, round-to-nearest-even; k >= K: +0
 * followed by 64 rows (2048 elements) of +0 (csrc/wrnn_tile_bf16.hip: what a lane loads, and why). */
int wrnn_debug_tile_bf16_pack(const float *W, int32_t rows, int32_t K, uint16_t *out, size_t cap);
/* Test hook, host only (no device, the HIP runtime is not touched): the packing routine of the tile-sparse view on ONE row-major matrix W [rows][K] of
 * `gates` gates (rows / gates a multiple of 16).  Returns the number of 16-column GROUPS of the packed lists (or WRNN_ERR_ARG) and fills
 *   tab   [rows / 16][2]        per block row: the first group of its list | its surviving columns n (ascending; groups: (n + 15) / 16)
 *   kept, total, admitted       surviving / all blocks; 1 when wrnn_pack_create admits this matrix to a view (at most 41 % survive: 100 * kept <= 41 * total), else 0
 * and, when cols and vals are non-NULL and the groups fit group_capacity,
 *   cols  [groups][4 kq][4 e]   the column of list entry 16 g + 4 e + kq of the block row that owns group g
 *   vals  [groups][64 l][4 e]   W[16 block row + (l & 15)][column of list entry 16 g + 4 e + (l >> 4)]
 * entries past n: value 0.0f, column = the last surviving one (a padded term is an exact no-op on finite activations); an empty list has no group. */
int wrnn_debug_tile_sparse_pack(const float *W, int32_t rows, int32_t K, int32_t gates, int32_t *tab, int32_t *cols, float *vals,
                                int32_t group_capacity, int32_t *kept, int32_t *total, int32_t *admitted);

/* Workspace (device bytes) wrnn_generate needs for this geometry under these options (NULL = defaults).  With the loop
 * kernel it does not grow with T: conditioning is produced in slabs (942 segments x 12,100 steps: < 1 GB). */
size_t wrnn_workspace_bytes(const wrnn_pack *p, const wrnn_geometry *g, const wrnn_options *opt);

/*
 * The loop: replaces fatchord_version.py:192-245 (state init, the `for i in range(seq_len)` body incl.
 * sample_from_discretized_mix_logistic / softmax+Categorical, and the stack/transpose gather).
 *
 *   mels_up  device [L, M]          un-folded up-sampled mel  (`mels` of :186 before the fold)
 *   aux      device [n_frames, 4A]  MelResNet output per FRAME (`aux` of :186 before Stretch2d repeats it)
 *   noise    device, the sampling noise in the order the reference draws it; NULL exactly when wrnn_options.noise_lib = 1:
 *              MOL: [T, 11*B]: per step 10*B uniforms (segment-major, mixture-minor; distribution.py:106)
 *                   followed by B uniforms (distribution.py:118), all U(1e-5, 1-1e-5)
 *              RAW: [T, B, C] Exp(1) variates (Categorical.sample -> multinomial)
 *   out      device [B, T]          the (B,T) tensor of :243 (samples in [-1,1]; RAW: 2*idx/(C-1)-1)
 *
 * Enqueues on `stream`; does not synchronise.  Call wrnn_status() after synchronising to learn whether
 * the kernels completed (bounded spins never hang: they give up and report).
 */
int wrnn_generate(const wrnn_pack *p, const wrnn_geometry *g, const float *mels_up, const float *aux,
                  const float *noise, float *out, void *workspace, size_t workspace_bytes, const wrnn_options *opt,
                  void *stream);

/*
 * The same loop over an explicit SEGMENT TABLE: segment b, step t reads conditioning position
 * p = seg_pos[b] + t; positions p >= seg_lim[b] are zero padding.  This is `fold_with_overlap`
 * (fatchord_version.py:293-340) applied to SEVERAL utterances whose un-folded conditioning was concatenated
 * (every utterance must start on a frame boundary: offset % hop == 0): utterance u at sample offset o_u with
 * L_u samples contributes segments with seg_pos = o_u + i*(target+overlap), seg_lim = o_u + L_u.  It is what
 * lets one launch serve a whole corpus shard (BASELINE config 4) -- the reference calls generate() once per
 * utterance (gen_wavernn.py:26-35).  seg_pos / seg_lim are HOST arrays of n_segments int32.
 *   mels_up device [L, M], aux device [n_frames, 4A] (concatenated), noise/out as in wrnn_generate with
 *   B = n_segments.
 */
int wrnn_generate_segments(const wrnn_pack *p, int32_t n_segments, int32_t T, const int32_t *seg_pos,
                           const int32_t *seg_lim, int32_t L, int32_t hop, int32_t n_frames,
                           const float *mels_up, const float *aux, const float *noise, float *out,
                           void *workspace, size_t workspace_bytes, const wrnn_options *opt, void *stream);
size_t wrnn_workspace_bytes_segments(const wrnn_pack *p, int32_t n_segments, int32_t T, int32_t n_frames,
                                     const wrnn_options *opt);

/*
 * The sampling noise of wrnn_options.noise_lib = 1 as a tensor: steps [t_begin, t_end) of n_segments segments in the layout `noise` has above
 * (MOL: [t_end - t_begin, 11 * n_segments], n_classes ignored; RAW: [t_end - t_begin, n_segments, n_classes]); row 0 is step t_begin.
 * Philox4x32-10 with key = seed and counter = (t, j / 4, id of the segment): word j % 4 of that block makes the value of index j -- MOL: j = 0..9 the
 * mixture-selection uniforms, j = 10 the logistic one, each a float32 in [1e-5, 1 - 1e-5]; RAW: j = class, an Exp(1) variate, finite and > 0
 * (the two formulas: csrc/wrnn_philox.h).  seg_id: HOST [n_segments] or NULL (segment b has id b).
 * wrnn_noise_fill: `out` is a DEVICE pointer (16-byte aligned); asynchronous on `stream`.  wrnn_noise_fill_host: `out` is a HOST pointer; computed by the
 * calling thread, the HIP runtime is not touched.  The MOL values of the two are bit-identical; the RAW values differ by the two logf implementations.
 */
int wrnn_noise_fill(int mode, int32_t n_segments, int32_t n_classes, int32_t t_begin, int32_t t_end, uint64_t seed, const uint64_t *seg_id,
                    float *out, int device, void *stream);
int wrnn_noise_fill_host(int mode, int32_t n_segments, int32_t n_classes, int32_t t_begin, int32_t t_end, uint64_t seed, const uint64_t *seg_id,
                         float *out);

/*
 * The loss of a teacher-forced call (appended to ABI v9: the symbols tell whether a library has them): -log p of the waveform a
 * wrnn_generate* call was fed through wrnn_options.force_x, from the fc3 outputs it left in wrnn_options.logits -- what the reference's training
 * and validation compute on `WaveRNN.forward` (train_wavernn.py:83, :123): MOL `discretized_mix_logistic_loss` (utils/distribution.py:16-84 with
 * its defaults num_classes = 65536, log_scale_min = log(1e-14)), RAW `F.cross_entropy`.  float32 arithmetic, like the reference's.
 *   logits   [T][n_segments][n_classes], exactly the tensor wrnn_options.logits received
 *   target   [n_segments][T], exactly the force_x tensor of that call: MOL the sample value in [-1, 1]; RAW the class value 2 idx / (C - 1) - 1
 *            (the class is recovered as rint((x + 1) (C - 1) / 2), exact for C <= 2048, and clamped into [0, C))
 *   seg_len  int32 [n_segments] or NULL (every step counts): step t of segment b counts iff t < seg_len[b] (values outside [0, T] are clamped)
 *   nll      NULL, or float32 [n_segments][T]: -log p of every counted step, 0 for every step past seg_len
 *   sum      float64 [n_segments]: the sum of the segment's counted per-step float32 values, accumulated in float64 in a fixed order (steps
 *            t = s mod S in step order for each of S slots -- MOL 64, RAW 16 --, then the slots in order) without atomics: two runs give the
 *            same bits, and a segment's values and sum do not depend on the other segments of the call (one workgroup per segment).
 * wrnn_nll: DEVICE pointers; asynchronous on `stream`; no allocation, no synchronisation.  wrnn_nll_host: the same struct with HOST pointers
 * (`stream` ignored), computed by the calling thread, the HIP runtime is not touched; the two differ by their expf / logf / log1pf and, within a
 * step, by the order of the sums over the mixtures / classes.  WRNN_ERR_ARG with a message, before anything is launched: a struct size
 * mismatch, a NULL logits / target / sum, MOL with n_classes != 30, RAW with n_classes outside 2..2048, n_segments < 1 or T < 1.  wrnn_nll without
 * a device: WRNN_ERR_NO_DEVICE, behind those checks.
 */
typedef struct wrnn_nll_call {
    uint32_t struct_bytes;
    int32_t mode;            /* WRNN_MODE_* */
    int32_t n_classes;       /* MOL: 30; RAW: 2..2048 */
    int32_t n_segments, T;
    const float *logits;
    const float *target;
    const int32_t *seg_len;
    float *nll;
    double *sum;
    void *stream;
} wrnn_nll_call;
int wrnn_nll(int device, const wrnn_nll_call *c);
int wrnn_nll_host(const wrnn_nll_call *c);

/* What wrnn_generate_segments WOULD run for this many segments under these options (kernel, split, rounds, slab length),
 * without launching anything.  `launches` is left 0. */
int wrnn_plan_segments(const wrnn_pack *p, int32_t n_segments, int32_t T, const wrnn_options *opt, wrnn_run_info *out);

/* Synchronises `stream`, reads the kernel status words from `workspace`.  WRNN_OK or WRNN_ERR_KERNEL. */
int wrnn_status(void *workspace, void *stream);

/* Test hook: one exchanged activation layer (0 h1, 1 h2, 2 y1, 3 y2, 4 RAW logits) of (cluster, slot) at ring position `ring`
 * (= step % 4) of the loop kernel's exchange buffer, un-permuted from MFMA-fragment order into host_out[16 segments][512].
 * Call after a run with the same (n_segments, T, n_frames, opt).  Synchronises the device. */
int wrnn_debug_read_exchange(const wrnn_pack *p, void *workspace, int32_t n_segments, int32_t T, int32_t n_frames,
                             const wrnn_options *opt, int cluster, int slot, int layer, int ring, float *host_out);

/* Test hook: everything the launch planner reads of a pack and its device.  wrnn_pack_create fills one per pack; a test may write one by
 * hand to plan for a device it does not have. */
typedef struct wrnn_plan_traits {
    int32_t struct_bytes;
    int32_t n_cus;             /* wrnn_device_cus() */
    int32_t mode, C;           /* WRNN_MODE_*, n_classes */
    int32_t generic;           /* non-shipped dims (wrnn_generic_kernel only) ... */
    int32_t gH, gF, gM, gA;    /* ... rnn, fc, feat, aux dims of such a pack (they appear in a message only) */
    int32_t sp_nbp;            /* 0: the GRU matrices are not block-sparse enough for wrnn_sparse_kernel; else the padded blocks per block row, 48 / 64.
                                  A GENERIC pack (wrnn_sparse_kernel never runs it): > 0: it has a tile-sparse view (WRNN_ALGO_TILE_SPARSE), sp_fc = 1: with fc1 / fc2;
                                  < 0: none, -(1 + 1001 m + f) names the first GRU matrix m (0 rnn1 ih, 1 rnn1 hh, 2 rnn2 ih, 3 rnn2 hh) that keeps more than
                                  41 % of its blocks and its surviving fraction f in 1/1000 (a message only); 0: none (gH % 16, or nothing recorded) */
    int32_t sp_max_blocks;     /* |wrnn_pack_sparse_blocks()| (a message only) */
    int32_t sp_fc;             /* bit 0: fc1 / fc2 are block-sparse too (wrnn_pack_sparse_fc_blocks() > 0).  Recorded; no planning decision reads it.
                                  bit 1 (a GENERIC pack): it has NO bf16 view although its dims pass the LDS rule (a weight rounds to +-inf): WRNN_ALGO_TILE_BF16
                                  refuses it.  Otherwise a generic pack has the view exactly when WRNN_ALGO_TILE admits its dims */
} wrnn_plan_traits;
/* What wrnn_plan_segments (`out`) and wrnn_workspace_bytes_segments (`workspace_bytes`) answer for a pack with these traits: the same
 * code, return codes and wrnn_last_error() texts, with neither a pack nor a device -- the HIP runtime is not touched.  A step range in
 * `opt` is validated as wrnn_generate_segments validates it (the other two ignore it). */
int wrnn_debug_plan(const wrnn_plan_traits *traits, int32_t n_segments, int32_t T, int32_t n_frames,
                    const wrnn_options *opt, wrnn_run_info *out, size_t *workspace_bytes);

/* Timer objects (see wrnn_options.timer).  wrnn_timer_ms synchronises on the recorded events and returns the SUM of the
 * loop-kernel launch durations of the last call that used the timer, including the calls that continued it with
 * t_begin > 0 (<0 if none); wrnn_timer_launches their count. */
int wrnn_timer_create(int device, wrnn_timer **out);
void wrnn_timer_destroy(wrnn_timer *t);
float wrnn_timer_ms(wrnn_timer *t);
int wrnn_timer_launches(const wrnn_timer *t);

/*
 * Pre-loop stage: `UpsampleNetwork.forward` (fatchord_version.py:82-89) = MelResNet (:31-48) + ResBlocks (:13-28) on
 * f32 MFMA, and the Stretch2d / box-filter up-sampling of the mel (:51-61, :73-80, :86-88).  Host pointers, float32,
 * row-major, in the reference's state-dict order (keys in comments, C = compute_dims, R = res_out_dims).
 */
typedef struct wrnn_pre_weights {
    int32_t feat_dims;            /* 80 */
    int32_t compute_dims;         /* C (shipped: 128) */
    int32_t res_out_dims;         /* R (shipped: 128) */
    int32_t res_blocks;           /* number of ResBlocks */
    int32_t pad;                  /* 2.  Any dims the reference's constructor takes (fatchord_version.py:64-71): (80, 128, 128, pad 2) run the f32-MFMA
                                     MelResNet kernel, everything else wrnn_resnet_generic_kernel (round 5) */
    int32_t upsample_factors[3];  /* (5, 5, 11) */
    const float *conv_in_w;       /* upsample.resnet.conv_in.weight (C, feat, 2*pad+1) */
    const float *bn_in;           /* upsample.resnet.batch_norm.{weight,bias,running_mean,running_var}: [4][C] */
    const float *res_w;           /* upsample.resnet.layers.{i}.{conv1,conv2}.weight: [res_blocks][2][C][C] */
    const float *res_bn;          /* upsample.resnet.layers.{i}.batch_norm{1,2}.{weight,bias,running_mean,running_var}: [res_blocks][2][4][C] */
    const float *conv_out_w;      /* upsample.resnet.conv_out.weight (R, C) */
    const float *conv_out_b;      /* upsample.resnet.conv_out.bias (R) */
    const float *up_w;            /* upsample.up_layers.{1,3,5}.weight, concatenated: (2*s0+1) + (2*s1+1) + (2*s2+1) taps */
} wrnn_pre_weights;
typedef struct wrnn_pre wrnn_pre;

int wrnn_pre_create(const wrnn_pre_weights *w, int device, wrnn_pre **out);
void wrnn_pre_destroy(wrnn_pre *p);
int wrnn_pre_hop(const wrnn_pre *p);                                   /* product of the upsample factors */
size_t wrnn_pre_workspace_bytes(const wrnn_pre *p, int32_t n_frames);
/* mel: device [feat][n_frames] (the (1, feat, N) tensor generate() receives, fatchord_version.py:169,183);
 * mels_up: device [n_frames*hop][feat]; aux: device [n_frames][R] (per FRAME: the x hop Stretch2d repeat of :83-85 is
 * left to the loop).  n_frames >= 1: ONE frame is the smallest utterance the stage takes (the `pad` frames each side are zeros it supplies itself);
 * n_frames * hop <= 2e9.  Several utterances: wrnn_pre_upsample_many below (or one call per utterance with offset output pointers).
 * Asynchronous on `stream`. */
int wrnn_pre_upsample(const wrnn_pre *p, const float *mel, int32_t n_frames, float *mels_up, float *aux,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same without the last Stretch2d + conv stage and its crop (ABI v6): mel_rows: device [(n_frames + 2 pad) * s0 * s1][feat], the input
 * of the last stage, which wrnn_duo_kernel then forms inside the loop (wrnn_options.mel_stage = 1); aux as above. */
int wrnn_pre_upsample_rows(const wrnn_pre *p, const float *mel, int32_t n_frames, float *mel_rows, float *aux,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Several utterances in ONE call (appended to ABI v9: the symbols tell whether a library has them): a host table of utterances, each written into its
 * slice of the concatenated outputs -- rows [up_row, up_row + n_frames * hop) of `mels_up` (rows_only: [up_row, up_row + (n_frames + 2 pad) * s0 * s1) of
 * the mel_rows buffer) and rows [aux_row, aux_row + n_frames) of `aux`.  With the shipped hparams (80 / 128 / 128, pad 2, factors 5, 5, 11) every stage is
 * ONE launch for all utterances: a workgroup finds (utterance, tile) through a small prefix table that the call stages and uploads into the workspace in
 * one copy; an utterance keeps the tiles and grids wrnn_pre_upsample gives it and every output element the same summation order, so the result is
 * BITWISE that of n_utt wrnn_pre_upsample / _rows calls.  Any other hparams: those n_utt calls, made here.  The slices must not overlap (not checked).
 * WRNN_ERR_ARG -- before anything is launched -- for a NULL table, n_utt < 1, an n_frames < 1, a NULL mel, a negative offset, or a workspace smaller
 * than wrnn_pre_workspace_bytes_many(same table, same rows_only) (0 for a bad table).  Asynchronous on `stream`; the table is read during the call only. */
typedef struct wrnn_pre_utt {
    const float *mel;             /* device [feat][n_frames] */
    int32_t n_frames;
    int32_t reserved;             /* 0 */
    int64_t up_row;               /* first row of this utterance in mels_up / mel_rows ([row][feat]) */
    int64_t aux_row;              /* first row (= frame) of this utterance in aux ([frame][R]) */
} wrnn_pre_utt;
size_t wrnn_pre_workspace_bytes_many(const wrnn_pre *p, const wrnn_pre_utt *utts, int32_t n_utt, int32_t rows_only);
int wrnn_pre_upsample_many(const wrnn_pre *p, const wrnn_pre_utt *utts, int32_t n_utt, int32_t rows_only, float *mels_up, float *aux,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Test hook: a handle holding the DIMS of `w` only (no device, no weights; no pointer of `w` is read): the size queries answer on it, and every entry
 * point that would launch returns WRNN_ERR_NO_DEVICE on it BEHIND its argument checks -- which is what it is for, on a host without a device. */
int wrnn_pre_debug_host_handle(const wrnn_pre_weights *w, wrnn_pre **out);
const char *wrnn_pre_last_error(void);

/*
 * Post-loop stage on the device, float64 like the reference: `.astype(np.float64)` (:245), `decode_mu_law` (utils/dsp.py:
 * 98-103; `lut` = the expansion of every class value, computed by the caller with the reference's numpy expression, or NULL
 * for MOL / mu_law off), `xfade_and_unfold` (:342-405; `fade_in` / `fade_out` = its two overlap-long float64 ramps) and the
 * truncation + tail fade of :255-258 (`tail` = linspace(1, 0, 20*hop)).  Utterance u owns segments
 * [first[u], first[u]+folds[u]) of `segments` [n][T] and writes out[out_off[u] .. out_off[u+1]) (= wave_len_u samples).
 * All pointers are DEVICE pointers.  batched = 0: one segment per utterance, no cross-fade.  Asynchronous on `stream`.
 */
int wrnn_post_unfold(const float *segments, int32_t T, int32_t n_utt, const int32_t *first, const int32_t *folds,
                     const int64_t *out_off, const double *lut, int32_t n_classes, const double *fade_in,
                     const double *fade_out, int32_t overlap, const double *tail, int32_t tail_len, int32_t batched,
                     double *out, void *stream);
const char *wrnn_post_last_error(void);

/*
 * The same stage for a RANGE OF STEPS of many ragged, unfolded utterances (appended to ABI v9: the symbols tell whether a library has them): what a
 * caller enqueues behind every step slice of a continued loop call (wrnn_options.t_begin / t_end) to hand finished audio on while the loop goes on --
 * `batch.generate_unbatched`, `WaveRNN.generate_stream`; INTEGRATION.md "Streaming unbatched audio".  Utterance u is row row[u] of `segments` (NULL:
 * row u), one UNFOLDED segment of wave_len[u] samples.  Element (u, t - t0) of the outputs, t in [t0, t1):
 *   t <  wave_len[u]             lut[class of the sample] (`decode_mu_law`) or (double)sample, as wrnn_post_unfold with batched = 0;
 *   t >= wave_len[u] - tail_len  ... times tail[t - (wave_len[u] - tail_len)]: ONE double multiply, in the order of wrnn_post_unfold (:256-258);
 *   t >= wave_len[u]             0.0.
 * out64 holds that double, out32 the double rounded to the nearest float32 (what `save_wav`'s `.astype(np.float32)` makes of it).  So the chunks of
 * [0, T) in step order, each cut at wave_len[u], ARE the waveform wrnn_post_unfold writes, bit for bit, for any t0 / t1 / T (no alignment asked).
 * wrnn_post_chunk: DEVICE pointers; one launch, asynchronous on `stream`; no allocation, no synchronisation, no workspace.  wrnn_post_chunk_host:
 * the same struct with HOST pointers (`stream` ignored), computed by the calling thread, the HIP runtime is not touched; the two give the same bits
 * (there is no transcendental in either).  WRNN_ERR_ARG with a message through wrnn_post_last_error(), before anything is launched: a struct size
 * mismatch, a NULL segments / wave_len / tail, both outputs NULL, n_utt < 1, a range that is not 0 <= t0 < t1 <= T, tail_len < 0, lut with
 * n_classes < 2; the host form also: a wave_len[u] < tail_len (the reference raises there, :258) or a negative row[u] -- the device form cannot read
 * them, its caller checks.  wave_len[u] > T is allowed: steps past T are never asked for.
 */
typedef struct wrnn_post_chunk_call {
    uint32_t struct_bytes;
    int32_t n_utt, T;            /* utterances; row length of `segments` */
    int32_t t0, t1;              /* steps [t0, t1), 0 <= t0 < t1 <= T */
    int32_t n_classes, tail_len; /* n_classes is read only with lut */
    const float  *segments;      /* [rows][T]: the loop's `out` */
    const int32_t *row;          /* [n_utt] row of utterance u, or NULL (row u) */
    const int32_t *wave_len;     /* [n_utt] */
    const double *lut;           /* mu-law expansion table or NULL, as wrnn_post_unfold */
    const double *tail;          /* [tail_len] = linspace(1, 0, 20*hop) */
    double *out64;               /* [n_utt][t1-t0] or NULL */
    float  *out32;               /* [n_utt][t1-t0] or NULL; at least one of the two */
    void *stream;
} wrnn_post_chunk_call;
int wrnn_post_chunk(const wrnn_post_chunk_call *c);
int wrnn_post_chunk_host(const wrnn_post_chunk_call *c);

/*
 * BASELINE config 3's caller, the Tacotron side (ids -> mel -> linear), in three steps: wrnn_taco_encode (embedding, encoder pre-net, encoder CBHG,
 * `encoder_proj`: reference models/tacotron.py:24-39, :403-404; once per sentence), wrnn_taco_decode (the decoder loop as one persistent
 * kernel, SURVEY.md section 8 row f3: it replaces the per-frame loop of `Tacotron.generate()`, :396-414, around `Decoder.forward`, :218-279;
 * on hardware since round 3, tests/test_gpu_config3.py compares it with the reference's own output, tests/golden/tacotron_decoder_200f.npz)
 * and wrnn_taco_postnet (the post-net CBHG and `post_proj`, :424-425).  The first and the last are declared further down (wrnn_taco_front).
 * All pointers are DEVICE pointers to contiguous float32 tensors in the reference's state-dict layouts (`decoder.*`).
 */
typedef struct wrnn_taco_weights {
    uint32_t struct_bytes;
    int32_t n_mels, prenet1, prenet2, decoder_dims, encoder_width, lstm_dims, attn_filters, attn_kernel;   /* 80 256 128 256 256 512 32 31 */
    const float *prenet_fc1_w, *prenet_fc1_b, *prenet_fc2_w, *prenet_fc2_b;               /* [256][80] [256] [128][256] [128] */
    const float *attn_rnn_w_ih, *attn_rnn_w_hh, *attn_rnn_b_ih, *attn_rnn_b_hh;           /* GRUCell [768][384] [768][256] [768] [768] */
    const float *attn_W_w, *attn_W_b, *attn_conv_w, *attn_L_w, *attn_L_b, *attn_v_w;      /* LSA: [256][256] [256] [32][2][31] [256][32] [256] [256] */
    const float *rnn_input_w, *rnn_input_b;                                               /* [512][512] [512] */
    const float *rnn1_w_ih, *rnn1_w_hh, *rnn1_b_ih, *rnn1_b_hh;                           /* LSTMCell [2048][512] x2, [2048] x2 */
    const float *rnn2_w_ih, *rnn2_w_hh, *rnn2_b_ih, *rnn2_b_hh;
    const float *mel_proj_w;                                                              /* [n_mels * max_r][512] */
} wrnn_taco_weights;

typedef struct wrnn_taco_call {
    uint32_t struct_bytes;
    int32_t n;               /* encoder positions (<= 1024) */
    int32_t r, max_r;        /* frames per decoder step (decoder.r) / of the mel_proj view (:262) */
    int32_t max_steps;       /* decoder steps at most (the reference's `steps` / r) */
    float stop_threshold;    /* :411 */
    const float *seq;        /* [n][256] encoder_seq (:403) */
    const float *seq_proj;   /* [n][256] encoder_seq_proj (:404) */
    float *mel_out;          /* [max_steps][n_mels][r]: frame block of every step */
    float *scores_out;       /* [max_steps][n]: attention of every step (:413) */
    int32_t *steps_done;     /* decoder steps run, including the one that met the stop test */
    void *workspace;         /* wrnn_taco_workspace_bytes() */
    size_t workspace_bytes;
    void *stream;
    int32_t variant;         /* 0 = auto; 1 = the flag-barrier kernel (weights re-read from L2 every step, any CU count);
                                2 = the register-resident kernel (128 co-resident workgroups, tagged exchange, r <= 8);
                                3 = 2 with per-layer shader clocks of workgroup 0 in the last 24 x 8 bytes of the workspace */
} wrnn_taco_call;

size_t wrnn_taco_workspace_bytes(void);
/* Asynchronous on `stream`.  WRNN_ERR_RESIDENCY if the cooperative grid is refused. */
int wrnn_taco_decode(int device, const wrnn_taco_weights *w, const wrnn_taco_call *c);
/* Synchronises `stream`; out4 = {failure flag, code, workgroup, barrier} of the decode that used `workspace` (all 0 = clean). */
int wrnn_taco_status(const void *workspace, unsigned *out4, void *stream);
const char *wrnn_taco_last_error(void);

/*
 * The decoder loop for a LIST of sentences in one launch (csrc/wrnn_taco_batch.hip, wrnn_taco_batch_kernel): the register-resident kernel of
 * variant 2 with a sentence dimension -- each layer of a step runs for every live sentence before the next layer, so a step costs its ten
 * exchange hops once, not once per sentence.  Sentence s decodes until its own stop test (:411) fires or it has run max_steps[s] steps; rows
 * of mel_out[s] / scores_out[s] past steps_done[s] are not touched.  mel_out[s], scores_out[s] and steps_done[s] are bit-identical to
 * wrnn_taco_decode(variant = 2) on that sentence alone.  Limits: 1..WRNN_TACO_BATCH_MAX sentences per call, 1..WRNN_TACO_BATCH_NMAX encoder
 * positions per sentence (longer sentences: wrnn_taco_decode), r <= 8, a device with >= 128 CUs (else WRNN_ERR_RESIDENCY: there is no
 * flag-barrier form of this kernel).  The arrays marked HOST are read during the call only.
 */
#define WRNN_TACO_BATCH_MAX 8
#define WRNN_TACO_BATCH_NMAX 256
typedef struct wrnn_taco_batch_call {
    uint32_t struct_bytes;
    int32_t n_sent;                    /* 1..WRNN_TACO_BATCH_MAX */
    int32_t r, max_r;                  /* as wrnn_taco_call */
    float stop_threshold;              /* :411 */
    const int32_t *n;                  /* HOST [n_sent]: encoder positions, 1..WRNN_TACO_BATCH_NMAX */
    const int32_t *max_steps;          /* HOST [n_sent]: per-sentence step limit (>= 1) */
    const float *const *seq, *const *seq_proj;   /* HOST [n_sent] of DEVICE [n_s][256] */
    float *const *mel_out;             /* HOST [n_sent] of DEVICE [max_steps_s][n_mels][r] */
    float *const *scores_out;          /* HOST [n_sent] of DEVICE [max_steps_s][n_s] */
    int32_t *steps_done;               /* DEVICE [n_sent]: decoder steps run per sentence */
    void *workspace;                   /* wrnn_taco_batch_workspace_bytes(n_sent) */
    size_t workspace_bytes;
    void *stream;
} wrnn_taco_batch_call;
/* 0 for an n_sent outside 1..WRNN_TACO_BATCH_MAX. */
size_t wrnn_taco_batch_workspace_bytes(int32_t n_sent);
/* Asynchronous on `stream`.  Every argument is validated before the device is touched (WRNN_ERR_ARG; wrnn_taco_last_error() names the sentence
 * and the limit).  wrnn_taco_status reads this workspace as it reads wrnn_taco_decode's. */
int wrnn_taco_decode_batch(int device, const wrnn_taco_weights *w, const wrnn_taco_batch_call *c);

/*
 * The TEACHER-FORCED decoder loop for a list of sentences: ground-truth-aligned (GTA) mels, the reference's `Tacotron.forward(x, m,
 * generate_gta=True)` (models/tacotron.py:310-368) at batch size 1 per sentence, in eval mode.  The PreNet input of decoder step k is column
 * k r - 1 of the sentence's own ground-truth mel `force_mel[s]` (the zero <GO> frame for k = 0), so a small pre-pass (wrnn_taco_prenet_kernel)
 * forms the PreNet output of every step of every sentence into the workspace, and the loop (wrnn_taco_batch_kernel<SMAX, true>) is the batched
 * kernel's step without the mel poll, the stop test and the two PreNet layers: eight exchange hops per step, not ten.  Sentence s runs exactly
 * steps_s = ceil(frames[s] / r) steps (there is no stop test) and writes steps_s rows of mel_out[s] / scores_out[s]; rows past them are not
 * touched.  Every sentence is decoded as if alone: its output does not depend on what rides along, and is bit-identical to the free-running
 * kernel's wherever the forced mel equals that kernel's own output.  Limits: those of wrnn_taco_decode_batch (1..WRNN_TACO_BATCH_MAX sentences
 * of 1..WRNN_TACO_BATCH_NMAX encoder positions, r <= 8, >= 128 CUs, else WRNN_ERR_RESIDENCY), 1..2^20 frames per sentence.  The arrays
 * marked HOST are read during the call only.
 */
typedef struct wrnn_taco_forced_call {
    uint32_t struct_bytes;
    int32_t n_sent;                    /* 1..WRNN_TACO_BATCH_MAX */
    int32_t r, max_r;                  /* as wrnn_taco_call */
    const int32_t *n;                  /* HOST [n_sent]: encoder positions, 1..WRNN_TACO_BATCH_NMAX */
    const int32_t *frames;             /* HOST [n_sent]: N_s >= 1 ground-truth frames; steps_s = ceil(N_s / r) */
    const float *const *seq, *const *seq_proj;   /* HOST [n_sent] of DEVICE [n_s][256] */
    const float *const *force_mel;     /* HOST [n_sent] of DEVICE [n_mels][N_s], the decoder's scale ([-4, 4]) */
    float *const *mel_out;             /* HOST [n_sent] of DEVICE [steps_s][n_mels][r] */
    float *const *scores_out;          /* HOST [n_sent] of DEVICE [steps_s][n_s] */
    void *workspace;                   /* wrnn_taco_forced_workspace_bytes(n_sent, frames, r) */
    size_t workspace_bytes;
    void *stream;
} wrnn_taco_forced_call;
/* The batched decoder's prefix and tagged vectors, then the PreNet table (128 floats per step).  0 for a bad table: n_sent outside
 * 1..WRNN_TACO_BATCH_MAX, frames NULL or outside 1..2^20, r outside 1..8. */
size_t wrnn_taco_forced_workspace_bytes(int32_t n_sent, const int32_t *frames, int32_t r);
/* Asynchronous on `stream` (the pre-pass launch, then the cooperative launch).  Every argument is validated before the device is touched
 * (WRNN_ERR_ARG; wrnn_taco_last_error() names the sentence and the limit).  wrnn_taco_status reads this workspace as it reads the others'. */
int wrnn_taco_decode_forced(int device, const wrnn_taco_weights *w, const wrnn_taco_forced_call *c);

/* The bidirectional GRU that ends a CBHG (reference models/tacotron.py:95, applied at :137: `x, _ = self.rnn(x)`), one sequence,
 * hidden size 128 (encoder and post-net of the reference's hparams): one persistent workgroup per direction with W_hh in
 * registers.  gi_* = W_ih x + b_ih for all frames (a plain GEMM: the caller's).  Errors: wrnn_taco_last_error(). */
typedef struct wrnn_bigru_call {
    uint32_t struct_bytes;
    int32_t T, hidden;                       /* frames; 128 */
    const float *gi_fwd, *gi_rev;            /* [T][3 hidden] (gates r, z, n as in nn.GRU) */
    const float *w_hh_fwd, *w_hh_rev;        /* [3 hidden][hidden] */
    const float *b_hh_fwd, *b_hh_rev;        /* [3 hidden] */
    float *out;                              /* [T][2 hidden]: forward | reverse, as nn.GRU(bidirectional=True) returns */
    void *stream;
} wrnn_bigru_call;
int wrnn_bigru(int device, const wrnn_bigru_call *c);
/* The same GRU for n_seq sequences that share one weight set, in ONE launch of (2, n_seq) workgroups (appended to ABI v9: the symbol tells whether
 * a library has it): sequence s owns rows [off_s, off_s + T[s]) of gi_fwd / gi_rev / out, off = the prefix sum of T; workgroup (direction, s)
 * runs the loop of wrnn_bigru on those rows, so out is bit-identical to n_seq wrnn_bigru calls.  No workgroup waits for another (not a
 * cooperative launch).  WRNN_ERR_ARG for a struct size mismatch, n_seq outside 1..WRNN_TACO_FRONT_MANY_MAX, a T[s] outside 1..2^20, or a NULL
 * buffer.  T is read during the call only. */
#define WRNN_TACO_FRONT_MANY_MAX 64
typedef struct wrnn_bigru_many_call {
    uint32_t struct_bytes;
    int32_t n_seq, hidden;                   /* 1..WRNN_TACO_FRONT_MANY_MAX; 128 */
    const int32_t *T;                        /* HOST [n_seq]: frames per sequence */
    const float *gi_fwd, *gi_rev;            /* [sum T][3 hidden], sequence after sequence */
    const float *w_hh_fwd, *w_hh_rev;        /* [3 hidden][hidden] */
    const float *b_hh_fwd, *b_hh_rev;        /* [3 hidden] */
    float *out;                              /* [sum T][2 hidden] */
    void *stream;
} wrnn_bigru_many_call;
int wrnn_bigru_many(int device, const wrnn_bigru_many_call *c);

/*
 * The rest of Tacotron inference around the decoder loop (csrc/wrnn_cbhg.hip): the embedding and the encoder pre-net, both CBHGs (reference
 * models/tacotron.py:57-139: conv bank of BatchNormConv :43-54, max-pool, two projections, residual, pre_highway, highways, the
 * bidirectional GRU through wrnn_bigru), `encoder_proj` and `post_proj`.  float32 throughout (f32 MFMA).  The weight pointers are DEVICE
 * pointers to contiguous float32 tensors in the reference's state-dict layouts; create copies and repacks them (they may be freed after it).
 * Supported: conv banks of 1..16, channel counts that are multiples of 16 (16..4096), highway / GRU width 128; anything else is
 * WRNN_ERR_ARG with a message.  Errors: wrnn_taco_last_error().
 */
typedef struct wrnn_cbhg_weights {
    int32_t K;                            /* conv bank size: widths 1..K (encoder 16, post-net 8) */
    int32_t in_channels;                  /* encoder 128, post-net 80 (n_mels) */
    int32_t proj1_channels;               /* conv_project1 outputs: 128 / 256 */
    int32_t proj2_channels;               /* conv_project2 outputs: 128 / 80; == in_channels (the residual) */
    int32_t channels;                     /* bank outputs per width, highway and GRU width: 128 */
    int32_t num_highways;                 /* 0..4 */
    const float *bank_conv_w[16];         /* conv1d_bank.{i}.conv.weight (channels, in_channels, i + 1) */
    const float *bank_bn_w[16], *bank_bn_b[16], *bank_bn_mean[16], *bank_bn_var[16];   /* conv1d_bank.{i}.bnorm.{weight,bias,running_mean,running_var} */
    const float *proj1_conv_w;            /* conv_project1.conv.weight (proj1_channels, K * channels, 3) */
    const float *proj1_bn_w, *proj1_bn_b, *proj1_bn_mean, *proj1_bn_var;
    const float *proj2_conv_w;            /* conv_project2.conv.weight (proj2_channels, proj1_channels, 3) */
    const float *proj2_bn_w, *proj2_bn_b, *proj2_bn_mean, *proj2_bn_var;
    const float *pre_highway_w;           /* pre_highway.weight (channels, proj2_channels); NULL exactly when proj2_channels == channels */
    const float *highway_w1[4], *highway_b1[4], *highway_w2[4], *highway_b2[4];        /* highways.{i}.{W1,W2}.{weight,bias} */
    const float *rnn_w_ih, *rnn_w_hh, *rnn_b_ih, *rnn_b_hh;                             /* rnn.{weight,bias}_{ih,hh}_l0: [384][128] x2, [384] x2 */
    const float *rnn_w_ih_rev, *rnn_w_hh_rev, *rnn_b_ih_rev, *rnn_b_hh_rev;             /* ..._l0_reverse */
} wrnn_cbhg_weights;

typedef struct wrnn_taco_front_weights {
    uint32_t struct_bytes;
    int32_t n_symbols, embed_dims;        /* encoder.embedding.weight (n_symbols, embed_dims): 148 x 256 */
    int32_t prenet1, prenet2;             /* encoder.pre_net.fc1 / fc2 outputs: 256 / 128 */
    int32_t encoder_proj_dims;            /* encoder_proj.weight (encoder_proj_dims, 2 channels): 256 */
    int32_t n_mels, fft_bins;             /* post_proj.weight (fft_bins, 2 channels): 80 / 80 */
    const float *embedding;
    const float *prenet_fc1_w, *prenet_fc1_b, *prenet_fc2_w, *prenet_fc2_b;
    const float *encoder_proj_w, *post_proj_w;
    wrnn_cbhg_weights encoder_cbhg;       /* encoder.cbhg.* */
    wrnn_cbhg_weights postnet;            /* postnet.* */
} wrnn_taco_front_weights;
typedef struct wrnn_taco_front wrnn_taco_front;     /* opaque and immutable: the repacked weights and the BatchNorm scale / shift pairs */

int wrnn_taco_front_create(const wrnn_taco_front_weights *w, int device, wrnn_taco_front **out);
void wrnn_taco_front_destroy(wrnn_taco_front *f);
/* bytes of caller-owned, 256-byte aligned workspace one call with this many rows (characters / frames) needs */
size_t wrnn_taco_front_workspace_bytes(const wrnn_taco_front *f, int32_t rows);
/* ids: device int32 [n] -> seq_out device [n][2 channels] (encoder_seq, :403), seq_proj_out device [n][encoder_proj_dims] (:404): what
 * wrnn_taco_call.seq / seq_proj take.  pre_rnn_out: NULL, or device [n][channels] that receives the highway output in front of the GRU
 * (a test hook).  Outputs 16-byte aligned.  Asynchronous on `stream`; no allocation, no synchronisation. */
int wrnn_taco_encode(const wrnn_taco_front *f, const int32_t *ids, int32_t n, float *seq_out, float *seq_proj_out, float *pre_rnn_out,
                     void *workspace, size_t workspace_bytes, void *stream);
/* mel: device [n_mels][N] (the decoder's frames, (n_mels, N) as `Tacotron.generate()` holds them) -> linear_out device [N][fft_bins]
 * (the reference returns its transpose; the vocoder takes it).  pre_rnn_out as above, [N][channels]. */
int wrnn_taco_postnet(const wrnn_taco_front *f, const float *mel, int32_t N, float *linear_out, float *pre_rnn_out,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Both for a LIST of 1..WRNN_TACO_FRONT_MANY_MAX sentences in one call (appended to ABI v9: the symbols tell whether a library has them).  Sentence s
 * owns rows [off_s, off_s + n_s) of every concatenated tensor -- ids, seq_out, seq_proj_out, linear_out, pre_rnn_out -- where off is the prefix sum of
 * the lengths; every row width the library supports is a multiple of 16 floats, so a sentence's slice is 16-byte aligned when the tensor is, and a
 * slice of seq_out / seq_proj_out is directly what wrnn_taco_batch_call.seq[s] / seq_proj[s] take.  Every stage is ONE launch for all sentences
 * (wrnn_*_many_kernel: a workgroup finds its sentence and its tile in a small table passed with the launch; the GRU runs as wrnn_bigru_many); tiles,
 * conv windows, the max-pool's padding and the residual are taken per sentence, so every output element sees the operands of the single-sentence call
 * in the same order: the outputs of sentence s are BIT-IDENTICAL to wrnn_taco_encode / wrnn_taco_postnet on that sentence alone, whatever rides along
 * and in whatever order, and rows outside a sentence's range are not touched.  Asynchronous on `stream`; no allocation, no synchronisation; `n`, `N`
 * and `mel` are read during the call only.  WRNN_ERR_ARG (the message names the sentence and the limit), before anything is launched, for a NULL
 * handle, table or output, n_sent outside 1..WRNN_TACO_FRONT_MANY_MAX, a length outside 1..2^20, a NULL mel[s], an output that is not 16-byte or a
 * workspace that is not 256-byte aligned; WRNN_ERR_WORKSPACE below wrnn_taco_front_workspace_bytes_many (which is 0 for a bad table). */
size_t wrnn_taco_front_workspace_bytes_many(const wrnn_taco_front *f, const int32_t *n, int32_t n_sent);
int wrnn_taco_encode_many(const wrnn_taco_front *f, const int32_t *ids /* DEVICE [sum n], sentence after sentence */,
                          const int32_t *n /* HOST [n_sent] */, int32_t n_sent,
                          float *seq_out /* DEVICE [sum n][2 channels] */, float *seq_proj_out /* DEVICE [sum n][encoder_proj_dims] */,
                          float *pre_rnn_out /* NULL or DEVICE [sum n][channels] */,
                          void *workspace, size_t workspace_bytes, void *stream);
int wrnn_taco_postnet_many(const wrnn_taco_front *f, const float *const *mel /* HOST [n_sent] of DEVICE [n_mels][N_s] */,
                           const int32_t *N /* HOST [n_sent] */, int32_t n_sent,
                           float *linear_out /* DEVICE [sum N][fft_bins] */, float *pre_rnn_out /* NULL or DEVICE [sum N][channels] */,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Test hook: a handle holding the DIMS of `w` only (no device, no weights; no weight pointer of `w` is read): the size queries answer on it, and
 * every entry point that would launch returns WRNN_ERR_NO_DEVICE on it BEHIND its argument checks.  wrnn_taco_front_destroy frees it. */
int wrnn_taco_front_debug_host_handle(const wrnn_taco_front_weights *w, wrnn_taco_front **out);

/* Self tests of the device primitives (MFMA fragment layout, inter-workgroup granule all-gather).
 * Synchronous.  WRNN_OK or an error with a message. */
int wrnn_selftest(int device, int which);
/* microseconds per all-gather round measured by the last wrnn_selftest(device, 2) (<0 if none) */
float wrnn_selftest_metric(void);

/*
 * TWO sentence groups per launch of the batched Tacotron decoder (appended to ABI v9: the symbols tell whether a library has them).  The
 * kernel of wrnn_taco_decode_batch / wrnn_taco_decode_forced is a grid of 128 workgroups, one per CU; a device of 256 CUs runs a second,
 * fully independent group of up to WRNN_TACO_BATCH_MAX sentences on its other 128 workgroups in the SAME cooperative launch (the GROUPED
 * instantiations of wrnn_taco_batch_kernel: 256 workgroups; a workgroup finds its group and its index within it from its block index).
 * calls[g] is an ordinary call struct with a workspace of its own (wrnn_taco_batch_workspace_bytes / wrnn_taco_forced_workspace_bytes of that
 * group); the groups share the weights and nothing else -- no exchange word, no barrier -- and a group's workgroups return when their own group
 * has no live sentence.  Every sentence's mel_out, scores_out and steps_done are BIT-IDENTICAL to the plain call on its group alone; rows past a
 * sentence's end are not touched; wrnn_taco_status reads each group's workspace separately.  n_groups == 1 IS the plain call.  For
 * n_groups == 2 every argument of every group is validated before the device is touched: the plain call's checks (the message prefixed
 * "group g: "), and WRNN_ERR_ARG for n_groups outside 1..WRNN_TACO_GROUPS_MAX, a NULL calls / calls[g], groups whose stream, r or max_r
 * differ, and workspaces whose byte ranges overlap.  WRNN_ERR_RESIDENCY on a device with fewer than 256 CUs, or one that cannot hold 256
 * workgroups of the kernel at once (asked before anything is enqueued: neither workspace has been written; decode the groups by two plain
 * calls).  Asynchronous on the stream, no allocation, no synchronisation: per group the memset of its status words and tags (forced: and its
 * PreNet pre-pass launch), then ONE cooperative launch.
 */
#define WRNN_TACO_GROUPS_MAX 2
int wrnn_taco_decode_batch_groups(int device, const wrnn_taco_weights *w, const wrnn_taco_batch_call *const *calls, int32_t n_groups);
int wrnn_taco_decode_forced_groups(int device, const wrnn_taco_weights *w, const wrnn_taco_forced_call *const *calls, int32_t n_groups);
/* Test hook: the grouped kernel's map of a block index 0..255 to (group 0..1, workgroup 0..127 within the group).  Returns the placement the
 * library was built with (0: contiguous halves; 1: interleaved, a group on four XCDs), -1 for a block outside the grid or a NULL output. */
int wrnn_debug_taco_group_of(int32_t block, int32_t *group, int32_t *local);

/*
 * A WATCHED call (appended to ABI v9: the symbols tell whether a library has them): wrnn_generate_segments on one of the kernels that are launched once
 * for all T steps -- wrnn_generic_kernel, wrnn_tile_kernel, wrnn_tile_sparse_kernel, wrnn_tile_bf16_kernel, wrnn_tile_wide_kernel -- which also publishes
 * how far it has got, so that finished audio can be handed on while it runs.  Arguments, behaviour and samples are those of wrnn_generate_segments;
 * besides, the call zeroes progress[0 .. W) on the stream in front of the launch (W = wrnn_watch_words), and every workgroup that writes `out` stores
 * t + 1 into ITS word after step t whenever (t + 1) % progress_every == 0 or t + 1 == T.  A word's value v says: steps [0, v) of that workgroup's rows of
 * `out` are complete and visible to a kernel or copy launched from now on (wrnn_generic_kernel: word b = segment b; the tile kernels: word g = segments
 * [16 g, 16 g + 16)).  So min over the W words = the columns of ALL of `out` that are final.  Readers are launched LATER, on another stream: copy the words
 * to the host, take the minimum m, then launch whatever reads out[:, :m] (wrnn_post_chunk, a copy).  Nothing may poll the words from inside a kernel, and
 * the loop kernel never reads them or waits for anybody: a caller that stops looking changes nothing.  Publishing costs an L2 write-back (microseconds):
 * progress_every = 64 keeps it far below a percent of these kernels' step times.  The words before the call are NOT zero until the stream reaches the
 * call's memset: order the first look behind an event recorded in front of the call, on words the caller has zeroed.
 * WRNN_ERR_ARG, before anything is queued, the message naming the cause and the kernel planned: a call that plans onto another kernel (the resumable
 * kernels -- wrnn_loop / _duo / _sparse / _chain_kernel -- stream through wrnn_options.t_begin / t_end instead; wrnn_stream_kernel does not stream), a NULL
 * `progress`, progress_every < 1, progress_words < W, a partial step range in `opt`.
 * wrnn_watch_words: W for such a call, with the same refusals of kernel and step range; no device is touched.
 */
int wrnn_generate_segments_watched(const wrnn_pack *p, int32_t n_segments, int32_t T, const int32_t *seg_pos,
                                   const int32_t *seg_lim, int32_t L, int32_t hop, int32_t n_frames,
                                   const float *mels_up, const float *aux, const float *noise, float *out,
                                   void *workspace, size_t workspace_bytes, const wrnn_options *opt, void *stream,
                                   unsigned *progress, int32_t progress_words, int32_t progress_every);
int wrnn_watch_words(const wrnn_pack *p, int32_t n_segments, int32_t T, const wrnn_options *opt, int32_t *words);
/* Test hook: every refusal of a watched call for a pack with these traits (wrnn_debug_plan's), with neither a pack nor a device.  have_progress: > 0 a
 * non-NULL `progress`, 0 a NULL one, < 0: answer as wrnn_watch_words (progress_words / progress_every are not looked at).  `words` (may be NULL) <- W. */
int wrnn_debug_watch(const wrnn_plan_traits *traits, int32_t n_segments, int32_t T, const wrnn_options *opt, int32_t have_progress,
                     int32_t progress_words, int32_t progress_every, int32_t *words);

#ifdef __cplusplus
}
#endif
#endif /* WAVERNN_AMD_H */
