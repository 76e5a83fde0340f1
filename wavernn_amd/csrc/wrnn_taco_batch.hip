// wrnn_taco_batch.hip -- wrnn_taco_batch_kernel: the register-resident Tacotron decoder loop of wrnn_taco.hip (wrnn_taco_resident_kernel) for up
// to WRNN_TACO_BATCH_MAX sentences in ONE cooperative launch (`wrnn_taco_decode_batch`).  A list of sentences (BASELINE config 3 reads six) is
// otherwise decoded one launch after the other, each step of each sentence paying ten dependent exchange hops on its own.
//
// Same grid (128 co-resident workgroups x 4 waves), same ownership (wave gw owns row / unit gw of every layer, lanes split K), same resident
// weight registers -- loaded once, used for every sentence -- and the same tagged 8-byte exchange {value, tag = step + 1} in two parity buffers,
// now per sentence: sentence s owns the entries [s * BV_END, (s + 1) * BV_END).  What changes is the ORDER of a step: layer L runs for all live
// sentences (stage every sentence's inputs with the polls of all sentences in flight together, compute, publish), then layer L + 1 -- ten hops
// per step, not ten per sentence -- and the row work of a layer is written as SMAX independent instruction streams (dot products and
// `wave_total` butterflies of all sentences first, the pointwise math after), so that one sentence's dependent latencies are filled by the others'.
// SMAX is a compile-time bound (instantiations 2, 4, 8; n_sent <= SMAX at run time): the row work of the slots past n_sent, and of sentences that
// have ended, is still executed (on stale LDS, results dropped) -- predicating it would split the streams again.
//
// Arithmetic: every formula and every summation order is that of wrnn_taco_resident_kernel (the helpers are shared, wrnn_taco.h), so a
// sentence's mel, attention and step count are BIT-IDENTICAL to decoding it alone with variant 2 (tests/test_gpu_taco_batch.py).  The pointwise
// lines the compiler contracts in the single kernel (GRU: n = tanh(gi + r gh), h' = (h - n) z + n; LSTM: c' = f c + i g) are written with explicit
// fmaf in the form the single kernel's ISA has -- c' = fma(f, c, i * g) -- because the default contraction depends on the inlining context.
// Everything else is compiled with contraction OFF: the residual x + h of the LSTM layers is a multiply and an add in the single kernel (h is
// published too) and was fused to x + sigm(o) * tanh(c) here by default -- 2.6e-9 on the mel, found by the bitwise test.
//
// Ends: sentence s is live until its own stop test (:411, on the polled mel block, as in the single kernel) fires or it reaches max_steps[s].
// Every workgroup derives the live mask from the same polled words by the same code (nothing about it is exchanged); a sentence that is not
// live is never polled or published again and its outputs are not touched.  The kernel returns when no sentence is live.
// WAR safety of the parity buffers is the single kernel's argument per sentence: while s is live every wave publishes an LSTM unit of s in
// every step.  (tests/test_taco_batch_exchange_model.py checks the protocol, the ends included, under adversarial timing.)
// Spins: a poll waits at most for the slowest workgroup's layer of eight sentences (tens of microseconds); SPIN_LIMIT iterations of a sleep
// and up to eight reloads are seconds.
//
// FORCED (the second template parameter; `wrnn_taco_decode_forced`): the teacher-forced form of the same step, for ground-truth-aligned mels
// (the reference's `Tacotron.forward(x, m, generate_gta=True)`, models/tacotron.py:310-368).  The PreNet's input of step k is column k r - 1 of the
// recording's own mel (<GO> for k = 0), known before the loop: wrnn_taco_prenet_kernel forms pre2[s][k][0..128) for every step of every
// sentence into a table in the workspace (the same row ownership, lane split, butterfly and fmaxf(x + b, 0) as L1 / L2 below: the same bits), and
// the loop starts at L3, which stages its PreNet half from that table with plain loads (the table is immutable while the loop runs).  There
// is no poll of the previous mel block, no stop test, no L1 / L2 and no PreNet weight registers; sentence s is live for exactly
// max_steps[s] = ceil(frames[s] / r) steps; the mel rows go to mel_out[s] only (nobody reads BV_MEL).  L3 .. L10 are the code below, unchanged.
// WAR safety of the parity buffers WITHOUT the mel poll: an entry of step t (buffer t & 1) is overwritten by a store of step t + 2, and its last
// reader is a staging of step t + 1 (the `ptag` polls of L3, L8, L9).  A wave stores for step t + 2 only after its workgroup has passed the
// L9 and L10 polls of step t + 1 (X2 and X3: 512 entries each, one per wave of the grid), and a wave publishes X2 / X3 of step t + 1 in L8 / L9
// only after its own workgroup's stagings of that layer and of every earlier one -- which include every read of a step-t entry (the latest:
// H2(t), staged in L9 of step t + 1 before X3(t + 1) is published, and no step-(t + 2) store precedes its workgroup's L10 poll of X3(t + 1)).
// Every wave publishes an LSTM unit of every live sentence in every step and every workgroup polls all of them, so the argument covers every
// workgroup and every live sentence; an ended sentence is neither stored nor polled.  (tests/test_taco_forced_exchange_model.py runs this
// order under adversarial timing; one buffer per vector fails there.)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../include/wavernn_amd.h"
#include "wrnn_device.h"
#include "wrnn_taco.h"

// (the spin loop's reload over the sentences is unrolled by a later pass than the one `#pragma unroll` asks -- 0 scratch, no indexed registers --
// and the earlier pass says so in every instantiation)
#pragma clang diagnostic ignored "-Wpass-failed"

namespace wrnn {

constexpr int B_SMAX = WRNN_TACO_BATCH_MAX, B_NMAX = WRNN_TACO_BATCH_NMAX;
static_assert(B_NMAX == NT, "one encoder position per thread in the normalisation, one per wave (gw < 256) in the score layer");
// tagged vectors of ONE sentence: offsets in 8-byte entries, [2 parity buffers][length]
constexpr int BL_MEL = T_NM * R_MAXR;
constexpr int BV_MEL = 0, BV_PRE1 = BV_MEL + 2 * BL_MEL, BV_PRE2 = BV_PRE1 + 2 * T_P1, BV_ATTNH = BV_PRE2 + 2 * T_P2, BV_CTX = BV_ATTNH + 2 * T_DD,
              BV_PQ = BV_CTX + 2 * T_DD, BV_S = BV_PQ + 2 * T_DD, BV_X = BV_S + 2 * B_NMAX, BV_X2 = BV_X + 2 * T_LD, BV_X3 = BV_X2 + 2 * T_LD,
              BV_H1 = BV_X3 + 2 * T_LD, BV_H2 = BV_H1 + 2 * T_LD, BV_END = BV_H2 + 2 * T_LD;

struct TacoBatchSent {
    const float *seq, *seq_proj;          // [n][256]
    float *mel_out, *scores_out;          // [max_steps][80][r], [max_steps][n]
    int n, max_steps;                     // (0, 0 in the slots past n_sent)
};
struct TacoBatchArgs {
    wrnn_taco_weights w;
    TacoBatchSent s[B_SMAX];              // the per-sentence table travels by value
    unsigned *uw;                         // the status words' block (as wrnn_taco_decode lays it out)
    unsigned long long *tv;               // tagged vectors [n_sent][BV_END]
    int *steps_done;                      // [n_sent]
    int n_sent, r, max_r;
    float stop_threshold;
};
// the forced form: + the PreNet table of the pre-pass, [pre_off[s] + step][T_P2] for sentence s
struct TacoForcedArgs : TacoBatchArgs {
    const float *pre2;
    int pre_off[B_SMAX];
};
template <bool FORCED> struct TacoArgsOf { typedef TacoBatchArgs type; };
template <> struct TacoArgsOf<true> { typedef TacoForcedArgs type; };

// ---------------- two groups per launch (`wrnn_taco_decode_batch_groups` / `wrnn_taco_decode_forced_groups`) ----------------
// The grouped launch has G_MAX * R_NWG workgroups: each group of R_NWG workgroups runs the step code below on an argument block of its own --
// sentence table, status words, tagged vectors, steps_done, r, threshold, PreNet table -- and shares nothing with the other group but the
// (read-only) weight tensors.  Nothing in this kernel waits for the whole grid: every wait is a poll of a tagged entry of the workgroup's own
// group, so a group's workgroups return when their group has no live sentence, however long the other one runs.
constexpr int G_MAX = WRNN_TACO_GROUPS_MAX;
static_assert(G_MAX == 2, "taco_group_of maps onto two groups");
template <bool FORCED> struct TacoGroupArgs { typename TacoArgsOf<FORCED>::type g[G_MAX]; };
template <bool FORCED, bool GROUPED> struct TacoKernArgsOf { typedef typename TacoArgsOf<FORCED>::type type; };
template <bool FORCED> struct TacoKernArgsOf<FORCED, true> { typedef TacoGroupArgs<FORCED> type; };

// Where the workgroups of a group sit (a speed question only: nothing below depends on where a workgroup runs).
//   0: contiguous halves -- group = block / 128.  Under the round-robin dispatch over the eight XCDs each group has 16 workgroups on every XCD.
//   1: interleaved -- group = bit 2 of (block mod 8): under that dispatch group 0 keeps to XCDs 0-3 and group 1 to XCDs 4-7, 32 workgroups each,
//      so a group's exchange stays within four XCDs.
// (DESIGN.md section 6 "Two sentence groups per launch" has the measurement behind the shipped value.)
#ifndef WRNN_TACO_GROUP_PLACEMENT
#define WRNN_TACO_GROUP_PLACEMENT 1
#endif
static_assert(WRNN_TACO_GROUP_PLACEMENT == 0 || WRNN_TACO_GROUP_PLACEMENT == 1, "placement 0 (contiguous) or 1 (interleaved)");
// block 0 .. G_MAX * R_NWG - 1 -> (group, local workgroup 0 .. R_NWG - 1): a bijection for either placement
__host__ __device__ __forceinline__ void taco_group_of(int block, int &group, int &local)
{
    if constexpr (WRNN_TACO_GROUP_PLACEMENT == 0) {
        group = block / R_NWG;
        local = block % R_NWG;
    } else {
        group = (block >> 2) & 1;
        local = (block >> 3) * 4 + (block & 3);
    }
}
template <bool GROUPED, class KA> __device__ __forceinline__ const auto &taco_group_args(const KA &ka, int group)
{
    if constexpr (GROUPED) return ka.g[group];
    else return ka;
}

// a value that is the same in every lane, moved to a scalar register
__device__ __forceinline__ float uni(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }

// No contraction of this kernel's own expressions: where the single kernel's ISA has a fused multiply-add the source below says fmaf, and where
// it has a multiply and an add (x + h of the residual LSTMs: h is published too) the two stay apart.  Left to the default, the compiler fuses
// x + sigm(o) * tanh(c) here and not there.
#pragma clang fp contract(off)

template <int SMAX, bool FORCED = false, bool GROUPED = false>
__global__ __launch_bounds__(NT, 1) void wrnn_taco_batch_kernel(const typename TacoKernArgsOf<FORCED, GROUPED>::type ka)
{
    // GROUPED: this workgroup's group and its index within it; everything below knows the group only through `a` and `wg`
    int grp = 0, lwg = (int)blockIdx.x;
    if constexpr (GROUPED) taco_group_of((int)blockIdx.x, grp, lwg);
    const typename TacoArgsOf<FORCED>::type &a = taco_group_args<GROUPED>(ka, grp);

    __shared__ __attribute__((aligned(16))) float xb[SMAX][2][1024];  // a layer's input vector(s); layers alternate the two buffers
    __shared__ __attribute__((aligned(16))) float melv[FORCED ? 1 : SMAX][BL_MEL]; // the previous step's mel block (stop test + prenet input)
    __shared__ __attribute__((aligned(16))) float ahv[SMAX][T_DD];    // attn_h of this step (query layer and rnn_input)
    __shared__ __attribute__((aligned(16))) float sc[SMAX][B_NMAX];   // scores of the step (raw, then normalised)
    __shared__ __attribute__((aligned(16))) float att[SMAX][B_NMAX];  // this workgroup's copy of the previous attention ...
    __shared__ __attribute__((aligned(16))) float cum[SMAX][B_NMAX];  // ... and of the cumulative attention (:205-206)
    __shared__ __attribute__((aligned(16))) float convT[2 * T_AK * T_AF];   // location conv weights, [tap of (channel, k)][filter]
    __shared__ __attribute__((aligned(16))) float LT[T_AF * T_DD];          // L weights, [filter][dim]
    __shared__ float red[SMAX][NW];
    __shared__ unsigned nbw[NW];
    __shared__ int misc[4];
    // (The score layer's per-wave window (62 floats) lives in xb[s][0][256 + 64 w ...) and its filter outputs (32) in xb[s][1][384 + 32 w ...): both
    // ranges are free at that point of a step and are re-staged before they are read again.  NOT xb[s][.][512 ...): the recurrent halves of the
    // GRU / LSTM inputs are not polled at step 0 and must still hold the zeros of the initial state.)

    const int tid = threadIdx.x, lane = tid & 63, wg = lwg;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);           // (scalar: the wave's rows, biases and cell states stay out of the vector registers)
    const int gw = wg * NW + w;
    const int gt = wg * NT + tid, NGT = R_NWG * NT;
    const int r = a.r, nmel = T_NM * a.r;
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(a.tv, (unsigned)a.n_sent * (unsigned)(BV_END * 8));
    unsigned *status = a.uw + U_STATUS;
    bool ok = true;

    // ---------------- resident weights (float4 chunk c of a row: k = 4 lane + 256 c), as in wrnn_taco_resident_kernel ----------------
    const int k0 = 4 * lane;
    // LEAN (the 8-sentence form): the rows used once per step by a single butterfly -- prenet, query, mel, the second chunk of the GRU's input
    // rows, v and the L bias -- are NOT resident: they are re-read every step (1 KB per wave and row, contiguous, from L2, in flight under the
    // layer's poll), because 200 weight registers and eight sentences' state do not fit 512 registers without scratch.  The values are the same.
    constexpr bool LEAN = SMAX > 4;
    const bool u256 = gw < T_DD, u128 = gw < T_P2;
#define LD_FC1() ldw4(a.w.prenet_fc1_w + (size_t)gw * T_NM + k0, u256 && k0 < T_NM)
#define LD_FC2() ldw4(a.w.prenet_fc2_w + (size_t)gw * T_P1 + k0, u128)
#define LD_GI1(q) ldw4(a.w.attn_rnn_w_ih + (size_t)((q) * T_DD + gw) * (T_DD + T_P2) + 256 + k0, u256 && k0 < T_P2)
#define LD_Q() ldw4(a.w.attn_W_w + (size_t)gw * T_DD + k0, u256)
#define LD_MP(c) ldw4(a.w.mel_proj_w + (size_t)((gw / r) * a.max_r + gw % r) * T_LD + 256 * (c) + k0, gw < nmel)
#define LD_V() ldw4(a.w.attn_v_w + k0, true)
#define LD_LB() ldw4(a.w.attn_L_b + k0, true)
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 w_fc1 = (LEAN || FORCED) ? z4 : LD_FC1();              // (FORCED: the PreNet ran in the pre-pass)
    const float4 w_fc2 = (LEAN || FORCED) ? z4 : LD_FC2();
    float4 g_i[3][2], g_h[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const size_t row = (size_t)(q * T_DD + gw);
        g_i[q][0] = ldw4(a.w.attn_rnn_w_ih + row * (T_DD + T_P2) + k0, u256);
        g_i[q][1] = LEAN ? z4 : LD_GI1(q);
        g_h[q] = ldw4(a.w.attn_rnn_w_hh + row * T_DD + k0, u256);
    }
    const float4 w_q = LEAN ? z4 : LD_Q();
    float4 w_ri[2], l1i[4][2], l1h[4][2], l2i[4][2], l2h[4][2], w_mp[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        w_ri[c] = ldw4(a.w.rnn_input_w + (size_t)gw * (2 * T_DD) + 256 * c + k0, true);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t row = (size_t)(q * T_LD + gw) * T_LD + 256 * c + k0;
            l1i[q][c] = ldw4(a.w.rnn1_w_ih + row, true); l1h[q][c] = ldw4(a.w.rnn1_w_hh + row, true);
            l2i[q][c] = ldw4(a.w.rnn2_w_ih + row, true); l2h[q][c] = ldw4(a.w.rnn2_w_hh + row, true);
        }
        w_mp[c] = LEAN ? z4 : LD_MP(c);
    }
    const float4 v_w0 = LEAN ? z4 : LD_V(), L_b0 = LEAN ? z4 : LD_LB();
    // biases of this wave's rows (wave-uniform)
    const float b_fc1 = u256 ? a.w.prenet_fc1_b[gw] : 0.f, b_fc2 = u128 ? a.w.prenet_fc2_b[gw] : 0.f;
    const float b_q = u256 ? a.w.attn_W_b[gw] : 0.f;
    float b_gi[3], b_gh[3], b_l1[4], b_l1h[4], b_l2[4], b_l2h[4];
#pragma unroll
    for (int q = 0; q < 3; ++q) { b_gi[q] = u256 ? a.w.attn_rnn_b_ih[q * T_DD + gw] : 0.f; b_gh[q] = u256 ? a.w.attn_rnn_b_hh[q * T_DD + gw] : 0.f; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        b_l1[q] = a.w.rnn1_b_ih[q * T_LD + gw]; b_l1h[q] = a.w.rnn1_b_hh[q * T_LD + gw];
        b_l2[q] = a.w.rnn2_b_ih[q * T_LD + gw]; b_l2h[q] = a.w.rnn2_b_hh[q * T_LD + gw];
    }
    const float b_ri = a.w.rnn_input_b[gw];

    // ---------------- per sentence: context columns (n <= 256: four positions per lane) and cell states.  (The projection row of position gw,
    // one float4 per lane and sentence, is re-read every step -- 1 KB per wave, contiguous, in flight under the poll of the query: eight of
    // them resident are what the register file of the 8-sentence form no longer holds.) ----
    int ns[SMAX];
    float seqc[SMAX][4];                                               // context dim gw: encoder_seq[pos = lane + 64 i][gw]
    float c1[SMAX], c2[SMAX];                                          // this wave's LSTM cell states (uniform over the lanes: kept in scalar registers)
    int dn[SMAX];                                                      // steps run (set when the sentence ends)
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        ns[s] = s < a.n_sent ? a.s[s].n : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) seqc[s][i] = (u256 && lane + 64 * i < ns[s]) ? a.s[s].seq[(size_t)(lane + 64 * i) * T_DD + gw] : 0.f;
        c1[s] = 0.f; c2[s] = 0.f; dn[s] = 0;
    }

    // ---------------- LDS: attention weights (transposed: conflict-free lane strides), zero state ----------------
    for (int k = tid; k < T_AF * 2 * T_AK; k += NT) convT[(k % (2 * T_AK)) * T_AF + k / (2 * T_AK)] = a.w.attn_conv_w[k];
    for (int k = tid; k < T_DD * T_AF; k += NT) LT[(k % T_AF) * T_DD + k / T_AF] = a.w.attn_L_w[k];
    for (int k = tid; k < SMAX * 2 * 1024; k += NT) (&xb[0][0][0])[k] = 0.f;
    if constexpr (!FORCED)
        for (int k = tid; k < SMAX * BL_MEL; k += NT) (&melv[0][0])[k] = 0.f;
    for (int k = tid; k < SMAX * B_NMAX; k += NT) { (&sc[0][0])[k] = 0.f; (&att[0][0])[k] = 0.f; (&cum[0][0])[k] = 0.f; (&ahv[0][0])[k] = 0.f; }
    if (tid < 4) misc[tid] = 0;
    __syncthreads();

    // the layers with several butterflies per sentence (GRU, scores, LSTMs) run in groups of G sentences: enough independent streams to fill the
    // pipeline, and the group's operands fit the register file (the pointwise math between two groups keeps the scheduler from merging them)
    constexpr int G = SMAX < 4 ? SMAX : 4;
    unsigned live = (1u << a.n_sent) - 1u;                             // bit s: sentence s is still decoding (wave-uniform, the same in every workgroup)
#define LV(s) ((live >> (s)) & 1u)

    // entries [ventry, ventry + cnt(s)) of every live sentence s -> dst + s * dstride, each polled until it carries `tag`; the loads of all
    // sentences are in flight together
    auto poll_in = [&](float *dst, int dstride, int ventry, int cntmax, auto cnt, unsigned tag, unsigned code) {
        for (int q0 = 0; q0 < cntmax; q0 += NT) {
            const int q = q0 + tid;
            u32x2 e[SMAX];
            bool in[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                in[s] = LV(s) && q < cnt(s);
                e[s] = u32x2{0u, tag};
                if (in[s]) e[s] = __builtin_amdgcn_raw_buffer_load_b64(vrs, (s * BV_END + ventry + q) * 8, 0, 16 /* sc1 */);
            }
            unsigned spins = 0;
            for (;;) {
                bool pend = false;
#pragma unroll
                for (int s = 0; s < SMAX; ++s) pend = pend || e[s].y != tag;
                if (!__any(pend)) break;
                if ((++spins & 255u) == 0u && (spins > SPIN_LIMIT || ld_agent32(status) != 0u)) {
                    if (lane == 0) report_failure(status, 0x900u | code, wg, tag, tid);
                    ok = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (e[s].y != tag) e[s] = __builtin_amdgcn_raw_buffer_load_b64(vrs, (s * BV_END + ventry + q) * 8, 0, 16 /* sc1 */);
            }
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (in[s]) dst[s * dstride + q] = __uint_as_float(e[s].x);
        }
    };
    auto pub = [&](int s, int ventry, float v, unsigned tag) {
        if (lane == 0) {
            const u32x2 e = {__float_as_uint(v), tag};
            __builtin_amdgcn_raw_buffer_store_b64(e, vrs, (s * BV_END + ventry) * 8, 0, 16 /* sc1 */);
        }
    };
#define FIXED(c) [&](int) { return (c); }
#define STAGED()                            \
    do {                                    \
        if (!ok) misc[0] = 1;               \
        __syncthreads();                    \
        if (misc[0] != 0) return;           \
    } while (0)

    for (int step = 0;; ++step) {
        const int p = step & 1;
        const unsigned tag = (unsigned)step + 1u, ptag = (unsigned)step;      // this step's entries / the previous step's
        // ---- ends by limit; the previous step's mel blocks: stop test of :411 per sentence ----------------------------------
#pragma unroll
        for (int s = 0; s < SMAX; ++s)
            if (LV(s) && step >= a.s[s].max_steps) { live &= ~(1u << s); dn[s] = step; }
        if (live == 0u) break;
        // (FORCED: L3 is the first staging of a step and writes xb[.][1], which the slower waves may still be reading in L10 of the step
        // before; the free-running form has the mel poll's barrier in between)
        if constexpr (FORCED) __syncthreads();
        // (wfc1 / wfc2 are declared at the step's scope, outside the `if constexpr` blocks: declared inside one, their lifetime ends at its brace
        // and the free-running instantiations allocate registers differently -- 3 to 22 more SGPR spills -- than before the FORCED parameter)
        const float4 wfc1 = (LEAN && !FORCED) ? LD_FC1() : w_fc1;
      if constexpr (!FORCED) {
        if (step > 0) poll_in(&melv[0][0], BL_MEL, BV_MEL + (p ^ 1) * BL_MEL, nmel, FIXED(nmel), ptag, 1);
        STAGED();
        {
            unsigned nb = 0u;
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                int notbelow = 0;
                for (int q = tid; q < nmel; q += NT) notbelow |= !(melv[s][q] < a.stop_threshold);
                if (__any(notbelow)) nb |= 1u << s;
            }
            if (lane == 0) nbw[w] = nb;
            __syncthreads();
            const unsigned any = (unsigned)__builtin_amdgcn_readfirstlane((int)((nbw[0] | nbw[1]) | (nbw[2] | nbw[3])));
            if (step > 0 && (step - 1) * r > 10) {                     // `(mel_frames < stop_threshold).all() and t > 10`, t = (step - 1) r
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (LV(s) && !((any >> s) & 1u)) { live &= ~(1u << s); dn[s] = step; }
            }
            if (live == 0u) break;
        }
        // ---- L1: PreNet fc1 on the last column of the previous block (<GO> = zeros) ----
        if (u256) {
            float t1[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                float x = 0.f;
                if (k0 < T_NM) {                                       // the last frame of the block: column j = r - 1 of rows m = k0 .. k0 + 3
                    x = fmaf(wfc1.x, melv[s][k0 * r + r - 1], x);
                    x = fmaf(wfc1.y, melv[s][(k0 + 1) * r + r - 1], x);
                    x = fmaf(wfc1.z, melv[s][(k0 + 2) * r + r - 1], x);
                    x = fmaf(wfc1.w, melv[s][(k0 + 3) * r + r - 1], x);
                }
                t1[s] = wave_total(x);
            }
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s)) pub(s, BV_PRE1 + p * T_P1 + gw, fmaxf(t1[s] + b_fc1, 0.f), tag);
        }
      }
        // ---- L2: PreNet fc2 ----
        const float4 wfc2 = (LEAN && !FORCED) ? LD_FC2() : w_fc2;
      if constexpr (!FORCED) {
        poll_in(&xb[0][0][0], 2048, BV_PRE1 + p * T_P1, T_P1, FIXED(T_P1), tag, 2);
        STAGED();
        if (u128) {
            float t2[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) t2[s] = wave_total(fma4(wfc2, xb[s][0] + k0, 0.f));
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s)) pub(s, BV_PRE2 + p * T_P2 + gw, fmaxf(t2[s] + b_fc2, 0.f), tag);
        }
      }
        // ---- L3: attention GRUCell on [context(t-1), prenet] with h = attn_h(t-1) (:233-235) ----
        float4 gi1[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) gi1[q] = LEAN ? LD_GI1(q) : g_i[q][1];
        if (step > 0) {
            poll_in(&xb[0][1][0], 2048, BV_CTX + (p ^ 1) * T_DD, T_DD, FIXED(T_DD), ptag, 3);
            poll_in(&xb[0][1][512], 2048, BV_ATTNH + (p ^ 1) * T_DD, T_DD, FIXED(T_DD), ptag, 3);
        }
        if constexpr (FORCED) {                                       // the PreNet half: this step's row of the pre-pass table (plain loads)
            float pv[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) pv[s] = (LV(s) && tid < T_P2) ? a.pre2[((size_t)a.pre_off[s] + (size_t)step) * T_P2 + tid] : 0.f;
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s) && tid < T_P2) xb[s][1][T_DD + tid] = pv[s];
        } else {
            poll_in(&xb[0][1][T_DD], 2048, BV_PRE2 + p * T_P2, T_P2, FIXED(T_P2), tag, 3);
        }
        STAGED();
        if (u256) {
#pragma unroll
          for (int s0 = 0; s0 < SMAX; s0 += G) {
            float gi[SMAX][3], gh[SMAX][3];
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    float x = fma4(g_i[q][0], xb[s][1] + k0, 0.f);
                    if (k0 < T_P2) x = fma4(gi1[q], xb[s][1] + 256 + k0, x);
                    gi[s][q] = wave_total(x) + b_gi[q];
                    gh[s][q] = wave_total(fma4(g_h[q], xb[s][1] + 512 + k0, 0.f)) + b_gh[q];
                }
            }
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
                const float rg = sigm(gi[s][0] + gh[s][0]), zg = sigm(gi[s][1] + gh[s][1]);
                const float ng = tanhf(fmaf(rg, gh[s][2], gi[s][2]));
                const float h = xb[s][1][512 + gw];
                if (LV(s)) pub(s, BV_ATTNH + p * T_DD + gw, fmaf(h - ng, zg, ng), tag);
            }
          }
        }
        // ---- L4: processed query (:193) ----
        const float4 wq = LEAN ? LD_Q() : w_q;
        poll_in(&ahv[0][0], T_DD, BV_ATTNH + p * T_DD, T_DD, FIXED(T_DD), tag, 4);
        STAGED();
        if (u256) {
            float t4[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) t4[s] = wave_total(fma4(wq, ahv[s] + k0, 0.f));
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s)) pub(s, BV_PQ + p * T_DD + gw, t4[s] + b_q, tag);
        }
        // ---- L5: location-sensitive scores (:194-203): wave gw is encoder position gw of every sentence ----
        const float4 v_w = LEAN ? LD_V() : v_w0, L_b = LEAN ? LD_LB() : L_b0;
        float4 spj[SMAX];                                              // encoder_seq_proj row of the position gw
#pragma unroll
        for (int s = 0; s < SMAX; ++s) spj[s] = ldw4(a.s[s].seq_proj + (size_t)gw * T_DD + k0, LV(s) && gw < ns[s]);
        poll_in(&xb[0][1][0], 2048, BV_PQ + p * T_DD, T_DD, FIXED(T_DD), tag, 5);
        STAGED();
        if (u256) {
            const int pos = gw;
#pragma unroll
          for (int s0 = 0; s0 < SMAX; s0 += G) {
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
                float *win = &xb[s][0][256 + 64 * w];
                if (lane < 2 * T_AK) {
                    const int c = lane / T_AK, k = lane % T_AK, idx = pos + k - T_AK / 2;
                    win[lane] = (idx >= 0 && idx < ns[s]) ? (c == 0 ? cum[s][idx] : att[s][idx]) : 0.f;
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane < T_AF) {
#pragma unroll
                for (int s = s0; s < s0 + G; ++s) {
                    const float *win = &xb[s][0][256 + 64 * w];
                    float x = 0.f;
                    for (int q = 0; q < 2 * T_AK; ++q) x = fmaf(convT[q * T_AF + lane], win[q], x);
                    xb[s][1][384 + T_AF * w + lane] = x;
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float t5[SMAX];
            float pl[G][4];
#pragma unroll
            for (int j = 0; j < G; ++j) { pl[j][0] = L_b.x; pl[j][1] = L_b.y; pl[j][2] = L_b.z; pl[j][3] = L_b.w; }
#pragma unroll 8
            for (int f = 0; f < T_AF; ++f) {                            // (one read of the L row per filter for the whole group; per sentence the
                const float4 lw = *reinterpret_cast<const float4 *>(LT + f * T_DD + k0);      //  sum runs over f in the single kernel's order)
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const float cv = xb[s0 + j][1][384 + T_AF * w + f];
                    pl[j][0] = fmaf(lw.x, cv, pl[j][0]); pl[j][1] = fmaf(lw.y, cv, pl[j][1]);
                    pl[j][2] = fmaf(lw.z, cv, pl[j][2]); pl[j][3] = fmaf(lw.w, cv, pl[j][3]);
                }
            }
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
                const float4 xq = *reinterpret_cast<const float4 *>(xb[s][1] + k0);
                const float4 sp = spj[s];
                float u = 0.f;
                u = fmaf(v_w.x, tanhf(xq.x + sp.x + pl[s - s0][0]), u);
                u = fmaf(v_w.y, tanhf(xq.y + sp.y + pl[s - s0][1]), u);
                u = fmaf(v_w.z, tanhf(xq.z + sp.z + pl[s - s0][2]), u);
                u = fmaf(v_w.w, tanhf(xq.w + sp.w + pl[s - s0][3]), u);
                t5[s] = wave_total(u);
            }
#pragma unroll
            for (int s = s0; s < s0 + G; ++s)
                if (LV(s) && pos < ns[s]) pub(s, BV_S + p * B_NMAX + pos, sigm(t5[s]), tag);
            __builtin_amdgcn_wave_barrier();
          }
        }
        // ---- L6: normalise (:204), this workgroup's copies of attention / cumulative (:205-206), context (:207) ----
        poll_in(&sc[0][0], B_NMAX, BV_S + p * B_NMAX, B_NMAX, [&](int s) { return ns[s]; }, tag, 6);
        STAGED();
        {
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                float part = 0.f;
                if (tid < ns[s]) part += sc[s][tid];
                part = wave_total(part);                               // the same tree in every workgroup: the same total everywhere
                if (lane == 0) red[s][w] = part;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                const float total = (red[s][0] + red[s][1]) + (red[s][2] + red[s][3]);
                if (LV(s) && tid < ns[s]) {
                    const float v = sc[s][tid] / total;
                    sc[s][tid] = v; att[s][tid] = v; cum[s][tid] += v;
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s))
                    for (int pos = gt; pos < ns[s]; pos += NGT) a.s[s].scores_out[(size_t)step * ns[s] + pos] = sc[s][pos];
            if (u256) {
                float t6[SMAX];
#pragma unroll
                for (int s = 0; s < SMAX; ++s) {
                    float x = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (64 * i < ns[s]) x = fmaf(sc[s][lane + 64 * i], seqc[s][i], x);
                    t6[s] = wave_total(x);
                }
#pragma unroll
                for (int s = 0; s < SMAX; ++s)
                    if (LV(s)) pub(s, BV_CTX + p * T_DD + gw, t6[s], tag);
            }
        }
        // ---- L7: rnn_input on [context, attn_h] (:246-247) ----
        poll_in(&xb[0][0][0], 2048, BV_CTX + p * T_DD, T_DD, FIXED(T_DD), tag, 7);
        STAGED();
        {
            float t7[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) t7[s] = wave_total(fma4(w_ri[1], ahv[s] + k0, fma4(w_ri[0], xb[s][0] + k0, 0.f)));
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s)) pub(s, BV_X + p * T_LD + gw, t7[s] + b_ri, tag);
        }
        // ---- L8: residual LSTMCell 1 (:249-251; ATen lstm_cell: gates i, f, g, o) ----
        poll_in(&xb[0][1][0], 2048, BV_X + p * T_LD, T_LD, FIXED(T_LD), tag, 8);
        if (step > 0) poll_in(&xb[0][1][T_LD], 2048, BV_H1 + (p ^ 1) * T_LD, T_LD, FIXED(T_LD), ptag, 8);
        STAGED();
#pragma unroll
        for (int s0 = 0; s0 < SMAX; s0 += G) {
            float g4[SMAX][4];
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    g4[s][q] = wave_total(fma4(l1i[q][1], xb[s][1] + 256 + k0, fma4(l1i[q][0], xb[s][1] + k0, 0.f))) + b_l1[q] +
                               wave_total(fma4(l1h[q][1], xb[s][1] + T_LD + 256 + k0, fma4(l1h[q][0], xb[s][1] + T_LD + k0, 0.f))) + b_l1h[q];
            }
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
                c1[s] = uni(fmaf(sigm(g4[s][1]), c1[s], sigm(g4[s][0]) * tanhf(g4[s][2])));
                const float h = sigm(g4[s][3]) * tanhf(c1[s]);
                if (LV(s)) {
                    pub(s, BV_H1 + p * T_LD + gw, h, tag);
                    pub(s, BV_X2 + p * T_LD + gw, xb[s][1][gw] + h, tag);
                }
            }
        }
        // ---- L9: residual LSTMCell 2 (:254-256) ----
        poll_in(&xb[0][0][0], 2048, BV_X2 + p * T_LD, T_LD, FIXED(T_LD), tag, 9);
        if (step > 0) poll_in(&xb[0][0][T_LD], 2048, BV_H2 + (p ^ 1) * T_LD, T_LD, FIXED(T_LD), ptag, 9);
        STAGED();
#pragma unroll
        for (int s0 = 0; s0 < SMAX; s0 += G) {
            float g4[SMAX][4];
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    g4[s][q] = wave_total(fma4(l2i[q][1], xb[s][0] + 256 + k0, fma4(l2i[q][0], xb[s][0] + k0, 0.f))) + b_l2[q] +
                               wave_total(fma4(l2h[q][1], xb[s][0] + T_LD + 256 + k0, fma4(l2h[q][0], xb[s][0] + T_LD + k0, 0.f))) + b_l2h[q];
            }
#pragma unroll
            for (int s = s0; s < s0 + G; ++s) {
                c2[s] = uni(fmaf(sigm(g4[s][1]), c2[s], sigm(g4[s][0]) * tanhf(g4[s][2])));
                const float h = sigm(g4[s][3]) * tanhf(c2[s]);
                if (LV(s)) {
                    pub(s, BV_H2 + p * T_LD + gw, h, tag);
                    pub(s, BV_X3 + p * T_LD + gw, xb[s][0][gw] + h, tag);
                }
            }
        }
        // ---- L10: mel_proj (:262-263): entry q = m r + j is row (m, j) of the (n_mels, max_r) view ----
        const float4 wmp0 = LEAN ? LD_MP(0) : w_mp[0], wmp1 = LEAN ? LD_MP(1) : w_mp[1];
        poll_in(&xb[0][1][0], 2048, BV_X3 + p * T_LD, T_LD, FIXED(T_LD), tag, 10);
        STAGED();
        if (gw < nmel) {
            float t10[SMAX];
#pragma unroll
            for (int s = 0; s < SMAX; ++s) t10[s] = wave_total(fma4(wmp1, xb[s][1] + 256 + k0, fma4(wmp0, xb[s][1] + k0, 0.f)));
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (LV(s)) {
                    if (lane == 0) a.s[s].mel_out[(size_t)step * nmel + gw] = t10[s];
                    if constexpr (!FORCED) pub(s, BV_MEL + p * BL_MEL + gw, t10[s], tag);
                }
        }
        for (int q = gw + R_NWV; q < nmel; q += R_NWV) {              // r >= 7 only: the rows past the 512 resident ones, from L2
            const float *wr = a.w.mel_proj_w + (size_t)((q / r) * a.max_r + q % r) * T_LD;
            const float4 wa = ldw4(wr + k0, true), wb = ldw4(wr + 256 + k0, true);
#pragma unroll
            for (int s = 0; s < SMAX; ++s) {
                const float x = wave_total(fma4(wb, xb[s][1] + 256 + k0, fma4(wa, xb[s][1] + k0, 0.f)));
                if (LV(s)) {
                    if (lane == 0) a.s[s].mel_out[(size_t)step * nmel + q] = x;
                    if constexpr (!FORCED) pub(s, BV_MEL + p * BL_MEL + q, x, tag);
                }
            }
        }
    }
    if constexpr (!FORCED) {
        if (gt == 0) {
#pragma unroll
            for (int s = 0; s < SMAX; ++s)
                if (s < a.n_sent) a.steps_done[s] = dn[s];
        }
    }
#undef STAGED
#undef FIXED
#undef LV
#undef LD_FC1
#undef LD_FC2
#undef LD_GI1
#undef LD_Q
#undef LD_MP
#undef LD_V
#undef LD_LB
}

// ---------------- the PreNet pre-pass of the forced form ----------------
// pre2[off_s + k][0..128) = PreNet(column k r - 1 of sentence s's forced mel; zeros for k = 0), for every step k of every sentence, before the
// loop.  One workgroup forms PN_CH consecutive steps of one sentence: fc1 into LDS, fc2 from LDS -- no exchange.  The arithmetic is L1 / L2 of
// wrnn_taco_batch_kernel: a wave owns a row, lane l holds its columns 4 l .. 4 l + 3 (ldw4), four fmaf in that order from 0 (fma4; the lanes
// past the 80 mel channels contribute 0), wave_total, fmaxf(x + b, 0) -- the bits the loop would have formed from the same input.  The PN_CH
// steps are independent instruction streams over one read of the row (as the sentences are in the loop kernel).
constexpr int PN_CH = 8;
struct TacoPrenetSent {
    const float *mel;                     // [n_mels][frames]
    int frames, steps, off, wg0;          // steps = ceil(frames / r); first table row; first workgroup of the sentence
};
struct TacoPrenetArgs {
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
    TacoPrenetSent s[B_SMAX];
    float *pre2;
    int n_sent, r;
};

__global__ __launch_bounds__(NT) void wrnn_taco_prenet_kernel(const TacoPrenetArgs a)
{
    __shared__ __attribute__((aligned(16))) float xin[PN_CH][T_NM];
    __shared__ __attribute__((aligned(16))) float p1[PN_CH][T_P1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int si = 0;
    for (int i = 1; i < B_SMAX; ++i)
        if (i < a.n_sent && (int)blockIdx.x >= a.s[i].wg0) si = i;
    const TacoPrenetSent sn = a.s[si];
    const int kf = ((int)blockIdx.x - sn.wg0) * PN_CH;                 // first step of this workgroup
    const int cnt = sn.steps - kf < PN_CH ? sn.steps - kf : PN_CH;
    for (int q = tid; q < PN_CH * T_NM; q += NT) {
        const int c = q / T_NM, m = q % T_NM, k = kf + c;
        xin[c][m] = (c < cnt && k > 0) ? sn.mel[(size_t)m * sn.frames + ((size_t)k * a.r - 1)] : 0.f;      // k r - 1 <= frames - 1 for k < steps
    }
    __syncthreads();
    const int k0 = 4 * lane;
    float4 wr = ldw4(a.fc1_w + (size_t)w * T_NM + k0, k0 < T_NM);
    for (int row = w; row < T_P1; row += NW) {
        const float4 wn = ldw4(a.fc1_w + (size_t)(row + NW) * T_NM + k0, row + NW < T_P1 && k0 < T_NM);      // the next row, in flight under this one
        const float b = a.fc1_b[row];
        float t[PN_CH];
#pragma unroll
        for (int c = 0; c < PN_CH; ++c) {
            float x = 0.f;
            if (k0 < T_NM) x = fma4(wr, xin[c] + k0, 0.f);
            t[c] = wave_total(x);
        }
#pragma unroll
        for (int c = 0; c < PN_CH; ++c)
            if (lane == c) p1[c][row] = fmaxf(t[c] + b, 0.f);
        wr = wn;
    }
    __syncthreads();
    wr = ldw4(a.fc2_w + (size_t)w * T_P1 + k0, true);
    for (int row = w; row < T_P2; row += NW) {
        const float4 wn = ldw4(a.fc2_w + (size_t)(row + NW) * T_P1 + k0, row + NW < T_P2);
        const float b = a.fc2_b[row];
        float t[PN_CH];
#pragma unroll
        for (int c = 0; c < PN_CH; ++c) t[c] = wave_total(fma4(wr, p1[c] + k0, 0.f));
#pragma unroll
        for (int c = 0; c < PN_CH; ++c)
            if (lane == c && c < cnt) a.pre2[((size_t)sn.off + kf + c) * T_P2 + row] = fmaxf(t[c] + b, 0.f);
        wr = wn;
    }
}

}  // namespace wrnn

// The code object holds the instantiations of wrnn_taco_batch_kernel in the order in which they are first named: pinned here (behind the
// namespace, so that the pre-pass kernel stays in front of them), and the host code below can name them in any order.
#define TACO_INSTANTIATE(FORCED, GROUPED)                                                                                         \
    template __global__ void wrnn::wrnn_taco_batch_kernel<2, FORCED, GROUPED>(const wrnn::TacoKernArgsOf<FORCED, GROUPED>::type); \
    template __global__ void wrnn::wrnn_taco_batch_kernel<4, FORCED, GROUPED>(const wrnn::TacoKernArgsOf<FORCED, GROUPED>::type); \
    template __global__ void wrnn::wrnn_taco_batch_kernel<8, FORCED, GROUPED>(const wrnn::TacoKernArgsOf<FORCED, GROUPED>::type);
TACO_INSTANTIATE(false, false)                                        // the plain calls: free-running, forced
TACO_INSTANTIATE(true, false)
TACO_INSTANTIATE(false, true)                                         // two groups per launch
TACO_INSTANTIATE(true, true)
#undef TACO_INSTANTIATE

using namespace wrnn;

constexpr int32_t FORCED_MAX_FRAMES = 1 << 20;

// workspace: the single-sentence decoder's prefix (wrnn_taco.h), then the tagged vectors of n_sent sentences
extern "C" size_t wrnn_taco_batch_workspace_bytes(int32_t n_sent)
{
    if (n_sent < 1 || n_sent > B_SMAX) return 0;
    return TACO_PREFIX_BYTES + (size_t)n_sent * BV_END * 8;
}

// the forced form (ground-truth-aligned mels): [the batched decoder's workspace | the PreNet table, (sum of steps) rows of T_P2 floats]
extern "C" size_t wrnn_taco_forced_workspace_bytes(int32_t n_sent, const int32_t *frames, int32_t r)
{
    if (n_sent < 1 || n_sent > B_SMAX || !frames || r < 1 || r > R_MAXR) return 0;
    size_t steps = 0;
    for (int s = 0; s < n_sent; ++s) {
        if (frames[s] < 1 || frames[s] > FORCED_MAX_FRAMES) return 0;
        steps += (size_t)((frames[s] + r - 1) / r);
    }
    return wrnn_taco_batch_workspace_bytes(n_sent) + steps * T_P2 * 4;
}

// ---------------- a decoder call, free-running or forced ----------------
// What the checks, the fill and the launch below read: the fields wrnn_taco_batch_call and wrnn_taco_forced_call share, the per-sentence step
// source, what only one form has, and the words in which the forms' messages differ.
struct TacoFormWords {
    const char *kernel;                   // "the ... kernel takes", "the ... decoder kernel needs"
    const char *longer;                   // where a sentence of more than B_NMAX positions goes
    const char *buffers, *sent_buffers;   // what a call, and a sentence of it, must not leave null
    const char *these, *ws_fn;            // "... sentences need N (the workspace function)"
};
static const TacoFormWords WORDS[2] = {
    {"batched", "; longer: wrnn_taco_decode", "n, max_steps, seq, seq_proj, mel_out, scores_out, steps_done and workspace",
     "seq, seq_proj, mel_out and scores_out", "", "wrnn_taco_batch_workspace_bytes"},
    {"forced", "", "n, frames, seq, seq_proj, force_mel, mel_out, scores_out and workspace", "seq, seq_proj, force_mel, mel_out and scores_out", "these ",
     "wrnn_taco_forced_workspace_bytes"}};

struct TacoCallView {
    const TacoFormWords *words;           // (null: the view of a null call)
    bool forced, size_ok;                 // size_ok: struct_bytes is the size of the public struct
    int32_t n_sent, r, max_r;
    const int32_t *n, *count;             // count[s]: max_steps[s] (free-running) or frames[s] (forced)
    const float *const *seq, *const *seq_proj, *const *force_mel;     // force_mel: forced only
    float *const *mel_out, *const *scores_out;
    int32_t *steps_done;                  // free-running only, as stop_threshold
    float stop_threshold;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
    int steps(int s) const { return forced ? (count[s] + r - 1) / r : count[s]; }
};

template <class Call> static TacoCallView view_shared(const Call *c, bool forced, const int32_t *count)
{
    TacoCallView v = {};
    v.words = &WORDS[forced]; v.forced = forced; v.size_ok = c->struct_bytes == sizeof(Call);
    v.n_sent = c->n_sent; v.r = c->r; v.max_r = c->max_r;
    v.n = c->n; v.count = count; v.seq = c->seq; v.seq_proj = c->seq_proj; v.mel_out = c->mel_out; v.scores_out = c->scores_out;
    v.workspace = c->workspace; v.workspace_bytes = c->workspace_bytes; v.stream = c->stream;
    return v;
}
static TacoCallView view_of(const wrnn_taco_batch_call *c)
{
    if (!c) return TacoCallView{};
    TacoCallView v = view_shared(c, false, c->max_steps);
    v.steps_done = c->steps_done; v.stop_threshold = c->stop_threshold;
    return v;
}
static TacoCallView view_of(const wrnn_taco_forced_call *c)
{
    if (!c) return TacoCallView{};
    TacoCallView v = view_shared(c, true, c->frames);
    v.force_mel = c->force_mel;
    return v;
}

// The argument checks of a call: everything is checked before the first HIP call.  `pre` is "" (a plain call) or "group g: " (a group of a
// groups call) in front of the message.
static int check_call(const wrnn_taco_weights *w, const TacoCallView &c, const char *pre)
{
    if (!w || !c.words) { taco_err("%snull argument", pre); return WRNN_ERR_ARG; }
    const TacoFormWords &words = *c.words;
    if (!c.size_ok || w->struct_bytes != sizeof(wrnn_taco_weights)) {
        taco_err("%sstruct size mismatch (header / library versions differ)", pre);
        return WRNN_ERR_ARG;
    }
    if (c.n_sent < 1 || c.n_sent > B_SMAX) {
        taco_err("%sn_sent=%d: a call decodes 1..%d sentences (WRNN_TACO_BATCH_MAX)", pre, c.n_sent, B_SMAX);
        return WRNN_ERR_ARG;
    }
    if (c.r < 1 || c.r > c.max_r || c.r > R_MAXR) {
        taco_err("%sr=%d max_r=%d: frames per step must be 1..min(max_r, %d)", pre, c.r, c.max_r, R_MAXR);
        return WRNN_ERR_ARG;
    }
    if (!c.n || !c.count || !c.seq || !c.seq_proj || (c.forced && !c.force_mel) || !c.mel_out || !c.scores_out || (!c.forced && !c.steps_done) ||
        !c.workspace) {
        taco_err("%snull buffer: %s are all required", pre, words.buffers);
        return WRNN_ERR_ARG;
    }
    for (int s = 0; s < c.n_sent; ++s) {
        if (c.n[s] < 1 || c.n[s] > B_NMAX) {
            taco_err("%ssentence %d: n=%d encoder positions, the %s kernel takes 1..%d (WRNN_TACO_BATCH_NMAX%s)", pre, s, c.n[s], words.kernel, B_NMAX,
                     words.longer);
            return WRNN_ERR_ARG;
        }
        if (c.forced && (c.count[s] < 1 || c.count[s] > FORCED_MAX_FRAMES)) {
            taco_err("%ssentence %d: frames=%d ground-truth frames, 1..%d", pre, s, c.count[s], FORCED_MAX_FRAMES);
            return WRNN_ERR_ARG;
        }
        if (!c.forced && c.count[s] < 1) {
            taco_err("%ssentence %d: max_steps=%d, at least 1", pre, s, c.count[s]);
            return WRNN_ERR_ARG;
        }
        if (!c.seq[s] || !c.seq_proj[s] || (c.forced && !c.force_mel[s]) || !c.mel_out[s] || !c.scores_out[s]) {
            taco_err("%ssentence %d: null buffer (%s are required)", pre, s, words.sent_buffers);
            return WRNN_ERR_ARG;
        }
    }
    const size_t need = c.forced ? wrnn_taco_forced_workspace_bytes(c.n_sent, c.count, c.r) : wrnn_taco_batch_workspace_bytes(c.n_sent);
    if (c.workspace_bytes < need) {
        taco_err("%sworkspace of %zu bytes, %s%d sentences need %zu (%s)", pre, c.workspace_bytes, words.these, c.n_sent, need, words.ws_fn);
        return WRNN_ERR_ARG;
    }
    return taco_check_geometry(w, pre);
}

// The argument blocks of a checked call: the loop's and, FORCED, the pre-pass's.  Returns the pre-pass's workgroup count (0 free-running).
template <bool FORCED> static int fill_args(typename TacoArgsOf<FORCED>::type &a, TacoPrenetArgs &pa, const wrnn_taco_weights *w, const TacoCallView &c)
{
    memset(&a, 0, sizeof a);
    a.w = *w;
    a.uw = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(c.workspace) + (size_t)A_END * 4);
    a.tv = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c.workspace) + TACO_PREFIX_BYTES);
    for (int s = 0; s < c.n_sent; ++s) {
        a.s[s].seq = c.seq[s]; a.s[s].seq_proj = c.seq_proj[s]; a.s[s].mel_out = c.mel_out[s]; a.s[s].scores_out = c.scores_out[s];
        a.s[s].n = c.n[s]; a.s[s].max_steps = c.steps(s);
    }
    a.steps_done = c.steps_done;
    a.n_sent = c.n_sent; a.r = c.r; a.max_r = c.max_r;
    a.stop_threshold = c.stop_threshold;
    int wgs = 0;
    if constexpr (FORCED) {
        memset(&pa, 0, sizeof pa);
        a.pre2 = pa.pre2 = reinterpret_cast<float *>(reinterpret_cast<char *>(c.workspace) + wrnn_taco_batch_workspace_bytes(c.n_sent));
        int off = 0;
        for (int s = 0; s < c.n_sent; ++s) {
            const int steps = c.steps(s);
            a.pre_off[s] = off;
            pa.s[s].mel = c.force_mel[s]; pa.s[s].frames = c.count[s]; pa.s[s].steps = steps; pa.s[s].off = off; pa.s[s].wg0 = wgs;
            off += steps;                                                  // (<= 8 * 2^20)
            wgs += (steps + PN_CH - 1) / PN_CH;
        }
        pa.fc1_w = w->prenet_fc1_w; pa.fc1_b = w->prenet_fc1_b; pa.fc2_w = w->prenet_fc2_w; pa.fc2_b = w->prenet_fc2_b;
        pa.n_sent = c.n_sent; pa.r = c.r;
    }
    return wgs;
}

// ---------------- two groups per launch ----------------
// calls[0] and calls[1] are ordinary calls with a workspace each; ONE cooperative launch of G_MAX * R_NWG workgroups decodes both (the GROUPED
// instantiations of wrnn_taco_batch_kernel: group g's R_NWG workgroups run the step code on calls[g]'s argument block).  SMAX comes from the
// larger group; the smaller group's slots past its n_sent are the slots past n_sent of any call.

extern "C" int wrnn_debug_taco_group_of(int32_t block, int32_t *group, int32_t *local)
{
    if (block < 0 || block >= G_MAX * R_NWG || !group || !local) return -1;
    int g = 0, l = 0;
    taco_group_of(block, g, l);
    *group = g; *local = l;
    return WRNN_TACO_GROUP_PLACEMENT;
}

// what the groups entry points check before the per-group checks: the count and the table
template <class Call> static int check_groups_table(const Call *const *calls, int32_t n_groups)
{
    if (n_groups < 1 || n_groups > G_MAX) {
        taco_err("n_groups=%d: a call decodes 1..%d groups (WRNN_TACO_GROUPS_MAX)", n_groups, G_MAX);
        return WRNN_ERR_ARG;
    }
    if (!calls) { taco_err("null argument: calls is a table of n_groups=%d call structs", n_groups); return WRNN_ERR_ARG; }
    for (int g = 0; g < n_groups; ++g)
        if (!calls[g]) { taco_err("group %d: null call (calls[0 .. n_groups) are all required)", g); return WRNN_ERR_ARG; }
    return WRNN_OK;
}

// ... and after them: what the groups of one launch must share, and what they must not
static int check_groups_pair(const TacoCallView &c0, const TacoCallView &c1)
{
    if (c0.stream != c1.stream) {
        taco_err("group 1: stream %p, group 0 has %p: the groups of a call ride ONE launch on one stream", c1.stream, c0.stream);
        return WRNN_ERR_ARG;
    }
    if (c0.r != c1.r || c0.max_r != c1.max_r) {
        taco_err("group 1: r=%d max_r=%d, group 0 has r=%d max_r=%d: the groups of a call share the weights, so r and max_r are equal", c1.r, c1.max_r,
                 c0.r, c0.max_r);
        return WRNN_ERR_ARG;
    }
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(c0.workspace), b1 = reinterpret_cast<uintptr_t>(c1.workspace);
    if (b0 < b1 + c1.workspace_bytes && b1 < b0 + c0.workspace_bytes) {
        taco_err("the workspaces of group 0 (%zu bytes at %p) and group 1 (%zu bytes at %p) overlap: every group needs a workspace of its own",
                 c0.workspace_bytes, c0.workspace, c1.workspace_bytes, c1.workspace);
        return WRNN_ERR_ARG;
    }
    return WRNN_OK;
}

template <bool FORCED, bool GROUPED> static const void *taco_kernel(int n_sent)
{
    return n_sent <= 2 ? (const void *)wrnn_taco_batch_kernel<2, FORCED, GROUPED> : n_sent <= 4 ? (const void *)wrnn_taco_batch_kernel<4, FORCED, GROUPED>
                                                                                                : (const void *)wrnn_taco_batch_kernel<8, FORCED, GROUPED>;
}

// The device's side of a call, before anything is enqueued.  A plain call: R_NWG CUs.  A grouped call: G_MAX * R_NWG workgroups of one per CU
// must be co-resident; the occupancy query is the one the runtime's cooperative launch repeats, so a refusal is found here, with neither
// workspace written.
static int taco_residency(int device, const void *kern, bool grouped, const char *kernel_word)
{
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { taco_err("hipGetDeviceProperties: %s", hipGetErrorString(e)); return WRNN_ERR_HIP; }
    if (!grouped) {
        if (prop.multiProcessorCount >= R_NWG) return WRNN_OK;
        taco_err("the %s decoder kernel needs >= %d CUs (one LSTM unit per wave of %d co-resident workgroups); device has %d", kernel_word, R_NWG, R_NWG,
                 prop.multiProcessorCount);
        return WRNN_ERR_RESIDENCY;
    }
    if (prop.multiProcessorCount < G_MAX * R_NWG) {
        taco_err("a launch of %d groups needs >= %d CUs (%d co-resident workgroups per group, one per CU); device has %d", G_MAX, G_MAX * R_NWG, R_NWG,
                 prop.multiProcessorCount);
        return WRNN_ERR_RESIDENCY;
    }
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, NT, 0);
    if (e != hipSuccess) { taco_err("hipOccupancyMaxActiveBlocksPerMultiprocessor: %s", hipGetErrorString(e)); return WRNN_ERR_HIP; }
    if ((long long)per_cu * prop.multiProcessorCount < G_MAX * R_NWG) {
        taco_err("a launch of %d groups needs %d co-resident workgroups; the device holds %d x %d", G_MAX, G_MAX * R_NWG, per_cu, prop.multiProcessorCount);
        return WRNN_ERR_RESIDENCY;
    }
    return WRNN_OK;
}

static void group_prefix(char (&pre)[16], int g, int n_groups)
{
    pre[0] = 0;
    if (n_groups > 1) snprintf(pre, sizeof pre, "group %d: ", g);
}

// One call of either form, of one group (the plain kernels on R_NWG workgroups) or of G_MAX (the GROUPED kernels): check, fill, launch.  The
// arguments of every group, and of the pair, are checked before the first HIP call.
template <bool FORCED, class Call> static int taco_decode(int device, const wrnn_taco_weights *w, const Call *const *calls, int n_groups)
{
    const bool grouped = n_groups > 1;
    TacoCallView c[G_MAX];
    char pre[16];
    for (int g = 0; g < n_groups; ++g) {
        group_prefix(pre, g, n_groups);
        c[g] = view_of(calls[g]);
        const int bad = check_call(w, c[g], pre);
        if (bad != WRNN_OK) return bad;
    }
    int bad = grouped ? check_groups_pair(c[0], c[1]) : WRNN_OK;
    if (bad != WRNN_OK) return bad;
    // ---- device ----
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e != hipSuccess) { taco_err("hipSetDevice: %s", hipGetErrorString(e)); return WRNN_ERR_HIP; }
    const int n_max = grouped && c[1].n_sent > c[0].n_sent ? c[1].n_sent : c[0].n_sent;
    const void *kern = grouped ? taco_kernel<FORCED, true>(n_max) : taco_kernel<FORCED, false>(n_max);
    bad = taco_residency(device, kern, grouped, c[0].words->kernel);
    if (bad != WRNN_OK) return bad;
    TacoGroupArgs<FORCED> ga;                                              // (a plain call's block is ga.g[0])
    TacoPrenetArgs pa[G_MAX];
    int wgs[G_MAX];
    for (int g = 0; g < n_groups; ++g) wgs[g] = fill_args<FORCED>(ga.g[g], pa[g], w, c[g]);
    hipStream_t stream = reinterpret_cast<hipStream_t>(c[0].stream);
    for (int g = 0; g < n_groups; ++g) {
        group_prefix(pre, g, n_groups);
        e = hipMemsetAsync(ga.g[g].uw, 0, (size_t)U_END * 4 + (size_t)c[g].n_sent * BV_END * 8, stream);               // tags 0: never a step's tag
        if (e != hipSuccess) { taco_err("%shipMemsetAsync: %s", pre, hipGetErrorString(e)); return WRNN_ERR_HIP; }
        if constexpr (FORCED) {
            hipLaunchKernelGGL(wrnn_taco_prenet_kernel, dim3(wgs[g]), dim3(NT), 0, stream, pa[g]);     // (one pre-pass launch per group: its table)
            e = hipGetLastError();
            if (e != hipSuccess) { taco_err("%slaunch of the PreNet pre-pass (%d workgroups): %s", pre, wgs[g], hipGetErrorString(e)); return WRNN_ERR_HIP; }
        }
    }
    void *params[] = {grouped ? (void *)&ga : (void *)&ga.g[0]};
    e = hipLaunchCooperativeKernel(kern, dim3(n_groups * R_NWG), dim3(NT), params, 0, stream);
    if (e != hipSuccess) { taco_err("cooperative launch of %d workgroups refused: %s", n_groups * R_NWG, hipGetErrorString(e)); return WRNN_ERR_RESIDENCY; }
    return WRNN_OK;
}

extern "C" int wrnn_taco_decode_batch(int device, const wrnn_taco_weights *w, const wrnn_taco_batch_call *c) { return taco_decode<false>(device, w, &c, 1); }

extern "C" int wrnn_taco_decode_forced(int device, const wrnn_taco_weights *w, const wrnn_taco_forced_call *c) { return taco_decode<true>(device, w, &c, 1); }

// (n_groups == 1 is the plain call: the same message, without a group in front)
extern "C" int wrnn_taco_decode_batch_groups(int device, const wrnn_taco_weights *w, const wrnn_taco_batch_call *const *calls, int32_t n_groups)
{
    const int bad = check_groups_table(calls, n_groups);
    return bad != WRNN_OK ? bad : taco_decode<false>(device, w, calls, n_groups);
}

extern "C" int wrnn_taco_decode_forced_groups(int device, const wrnn_taco_weights *w, const wrnn_taco_forced_call *const *calls, int32_t n_groups)
{
    const int bad = check_groups_table(calls, n_groups);
    return bad != WRNN_OK ? bad : taco_decode<true>(device, w, calls, n_groups);
}
