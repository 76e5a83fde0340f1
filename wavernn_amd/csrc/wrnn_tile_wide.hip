// wrnn_tile_wide.hip -- wrnn_tile_kernel (wrnn_tile.hip: dataflow, pack, LDS carve, arithmetic) with the ROWS of every matrix stage spread over a CLUSTER of
// W = 2, 4 or 8 workgroups per tile of up to 16 segments (WRNN_ALGO_TILE with wrnn_options.clusters = W; on request only).
//
// Division   workgroup (tile g, member m) = block g W + m.  Every member keeps the tile's full activation vectors in LDS (tile's carve).  A matrix stage
//            -- I, rnn1, rnn2, fc1, fc2, RAW's fc3 -- has U = ceil(rows / 16) UNITS of 16 consecutive rows; member m computes units [U m / W, U (m + 1) / W), a
//            contiguous run that may be empty, wave w of it every 8th.  A unit is ONE 16-row MFMA tile in the one-dword form (lane l reads
//            XT[(k0 + (l >> 4)) ld + row0 + (l & 15)]) on ONE accumulator in ascending k: the chain of wrnn_tile_kernel's interleaved tiles element for element
//            (a row of A touches that row of D only), so the samples and logits are tile's bit for bit whatever W is.  MoL's fc3 (30 rows) and both samplers
//            run on every member, in tile's code; every member derives the same x_t; member 0 writes `out`, the owner of a row its dbg_logits.
// Hand-off   per (tile, stage) ONE buffer [rows][16] in the workspace and W flag words.  A member stores its rows write-through (sc1), every storing wave
//            drains (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, one lane stores the member's flag = epoch (agent-scope atomic).  Wave 0 of every
//            member polls the W flags of the stage, relaxed, with s_sleep, until all equal the epoch; ONE agent-scope acquire follows the match, and every
//            load of the payload is an sc1 load besides.  Then the workgroup copies the WHOLE vector into LDS with the pointwise pass tile runs there
//            (h <- h', x1 = xi + h1, ...).  epoch = step * stages + stage + 1, counted within the call; the flag block is zeroed on the stream in front of
//            every launch.  No assumption on dispatch order or on which XCD a member runs.
// Re-use     a member publishes stage s of step t + 1 only after it has copied stage s - 1 of step t + 1 (stage S - 1 of step t for s = 0), which needs every
//            member's flag of that stage, which each of them stored -- in program order -- after its own copy of stage s of step t had finished (its loads
//            landed in LDS in front of a barrier).  So with at least two stages one buffer per (tile, stage) is never overwritten while a member still reads
//            it; tests/test_tile_wide_exchange_model.py runs the argument under adversarial timing and shows the shortcuts that break it.
// Failure    every spin is bounded (SPIN_LIMIT): the poller reports through the status words (wrnn_status -> WRNN_ERR_KERNEL) and its workgroup leaves; a
//            poller that sees a raised status word leaves too.  The launch is cooperative: W members that cannot be co-resident are refused, not hung.
#include "wrnn_tile_dev.h"

namespace wrnn {

size_t tile_lds_bytes(int H, int F, int M, int A, int C);        // wrnn_tile.hip: the carve is tile's

constexpr int WIDE_MAXW = 8;           // members per cluster: one 32-byte line of flags per (tile, stage)
constexpr int WIDE_STAGES = 6;          // I, rnn1, rnn2, fc1, fc2, RAW fc3 (MOL: five)

struct WideArgs {
    float *xbuf;                        // [tiles][WIDE_STAGES][xstride] floats: the stages' output vectors as [row][16 segments]
    unsigned *flags;                    // [tiles][WIDE_STAGES][WIDE_MAXW], zeroed in front of every launch
    unsigned *status;                   // [STATUS_WORDS]
    int W, xstride;
};

// NG 16-row tiles (consecutive rows, one dword per lane) of one k-major matrix against one activation vector over k in [0, K); tile g starts at row
// row0 + g * gstride.  ONE accumulator per tile, k ascending: tile_dot's V = 4 chain.  The operands of the next D k-steps ride in a register ring as there.
template <int NG, int D>
__device__ __forceinline__ void wide_dot(const float *WT, int ld, int gstride, int row0, int K, const float *act, int lane, f32x4 (&out)[NG])
{
    const int i = lane & 15, kq = lane >> 4;
    const float *bp = act + kq * SEG + i;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(WT, (unsigned)K * (unsigned)ld * 4u);
    const int voff = (kq * ld + row0 + i) * 4;
    const int nfull = K >> 2, sstep = 16 * ld;
    float x[D][NG], bv[D];
#pragma unroll
    for (int g = 0; g < NG; ++g) out[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto fill = [&](int d, int j) {
#pragma unroll
        for (int g = 0; g < NG; ++g) x[d][g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + g * gstride * 4, j * sstep, 0));
        bv[d] = bp[j * 4 * SEG];
    };
    auto use = [&](int d) {
#pragma unroll
        for (int g = 0; g < NG; ++g) out[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[d][g], bv[d], out[g], 0, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nfull) fill(d, d);
    int j0 = 0;
    for (; j0 + 2 * D <= nfull; j0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) { use(d); fill(d, j0 + d + D); }
    }
    for (; j0 < nfull; j0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (j0 + d < nfull) {
                use(d);
                if (j0 + d + D < nfull) fill(d, j0 + d + D);
            }
    }
    if (K & 3) {        // the K tail: k >= K supplies 0, read from a clamped address
        const int k = 4 * nfull + kq;
        const float b = bp[nfull * 4 * SEG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float xt = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, ((k < K ? k : K - 1) * ld + row0 + i + g * gstride) * 4, 0, 0));
            out[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(k < K ? xt : 0.f, b, out[g], 0, 0, 0);
        }
    }
}

// the hand-off buffer of one (tile, stage): stores and loads, all write-through / L1-bypassing (sc1)
__device__ __forceinline__ void wide_put(__amdgpu_buffer_rsrc_t xs, int r, int seg, float y)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(y), xs, (r * SEG + seg) * 4, 0, 16 /* sc1 */);
}

// this member's units of a stage with R rows
__device__ __forceinline__ void wide_share(int R, int m, int W, int &u0, int &u1)
{
    const int U = (R + 15) >> 4;
    u0 = U * m / W; u1 = U * (m + 1) / W;
}

// one Linear stage, units [u0, u1): [relu](XT . act + bias) -> the stage's buffer
template <bool RELU>
__device__ __forceinline__ void wide_linear(const float *WT, const float *bias, int R, int K, const float *act, __amdgpu_buffer_rsrc_t xs, int u0, int u1, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4;
    for (int u = u0 + w; u < u1; u += TNW) {
        f32x4 acc[1];
        wide_dot<1, 16>(WT, R, 0, u * 16, K, act, lane, acc);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = u * 16 + q4 + v;
            if (r < R) { const float y = acc[0][v] + bias[r]; wide_put(xs, r, seg, RELU ? fmaxf(y, 0.f) : y); }
        }
    }
}

// one GRU stage, units [u0, u1): the new h -> the stage's buffer
__device__ __forceinline__ void wide_gru(const float *WiT, const float *WhT, const float *bi, const float *bh, int H, int K1, const float *x, const float *hs,
                                         __amdgpu_buffer_rsrc_t xs, int u0, int u1, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4;
    for (int un = u0 + w; un < u1; un += TNW) {
        f32x4 gi[3], gh[3];
        wide_dot<3, 8>(WiT, 3 * H, H, un * 16, K1, x, lane, gi);
        wide_dot<3, 8>(WhT, 3 * H, H, un * 16, H, hs, lane, gh);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int u = un * 16 + q4 + v;
            if (u < H)
                wide_put(xs, u, seg, gru_update(gi[0][v] + bi[u], gi[1][v] + bi[H + u], gi[2][v] + bi[2 * H + u], gh[0][v] + bh[u], gh[1][v] + bh[H + u],
                                                gh[2][v] + bh[2 * H + u], hs[u * SEG + seg]));
        }
    }
}

// Publish: every storing wave has drained its sc1 stores, the workgroup has met, ONE lane stores the member's flag.
__device__ __forceinline__ void wide_signal(unsigned *flag, unsigned epoch, int tid)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Consume: wave 0 polls the W flags of the stage (lane m reads member m's), relaxed; one agent-scope acquire after the match.  The verdict goes through the
// LDS word `dead` to the whole workgroup (behind a barrier): false = leave (the spin ran out -- reported -- or another workgroup has reported).
__device__ __forceinline__ bool wide_wait(const unsigned *flags, int W, unsigned epoch, unsigned *status, unsigned code, int t, float *dead, int tid)
{
    if (tid < 64) {
        bool ok = true;
        for (unsigned spins = 0;;) {
            const unsigned v = tid < W ? ld_agent32(flags + tid) : epoch;
            if (__all(v == epoch)) break;
            if ((++spins & 255u) == 0u) {
                const bool out = spins > SPIN_LIMIT;
                if (out || ld_agent32(status) != 0u) {
                    if (out && tid == 0) report_failure(status, code, blockIdx.x, (unsigned)t, epoch);
                    ok = false;
                    break;
                }
            }
            __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) *dead = ok ? 0.f : 1.f;
    }
    __syncthreads();
    return *dead == 0.f;
}

// MODE: 0 RAW, 1 MOL (C == 30)
template <int MODE>
__global__ __launch_bounds__(TNT) void wrnn_tile_wide_kernel(const GenArgs a, const WideArgs x)
{
    extern __shared__ __attribute__((aligned(16))) float tsm[];
    const int H = a.H, F = a.F, M = a.M, A = a.A, C = a.C, T = a.T, B = a.B;
    const int K0 = 1 + M + A, HF = (H > F ? H : F) + A;
    float *in0 = tsm, *va = in0 + r4(K0) * SEG, *vb = va + r4(HF) * SEG, *h1s = vb + r4(HF) * SEG, *h2s = h1s + r4(H) * SEG, *red = h2s + r4(H) * SEG;
    float *dead = red + TRED - 1;           // the pollers' verdict: a word of the sampler scratch, which is idle between the samplers
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, seg = lane & 15, q4 = (lane >> 4) * 4;
    const int W = x.W, g = blockIdx.x / W, m = blockIdx.x - g * W;
    const int b0 = g * SEG, nb = (B - b0 < SEG) ? B - b0 : SEG;
    constexpr int S = MODE == 1 ? 5 : 6;
    unsigned *const flags = x.flags + (size_t)g * WIDE_STAGES * WIDE_MAXW;
    float *const xt = x.xbuf + (size_t)g * WIDE_STAGES * x.xstride;
    const unsigned xbytes = (unsigned)x.xstride * 4u;
    // h1 = h2 = 0, x_{-1} = 0; the padding rows and the dead columns stay 0 for the whole run
    for (int i = tid; i < (int)(red - tsm) + TRED; i += TNT) tsm[i] = 0.f;
    __syncthreads();

// stage s: publish, wait, and the buffer as `xs` for the copy that follows
#define WIDE_HANDOFF(s)                                                                                                                        \
    wide_signal(flags + (s) * WIDE_MAXW + m, (unsigned)(t * S + (s) + 1), tid);                                                                \
    if (!wide_wait(flags + (s) * WIDE_MAXW, W, (unsigned)(t * S + (s) + 1), x.status, 0xA00u | (unsigned)(s), t, dead, tid)) return;
#define WIDE_XS(s) make_rsrc(xt + (size_t)(s) * x.xstride, xbytes)
// 16-byte sc1 loads of the first n floats (n a multiple of 16) of the stage's buffer
#define WIDE_COPY(xs, n, i, q) for (int i = tid * 4; i < (n); i += TNT * 4) { const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(xs, i * 4, 0, 16 /* sc1 */);
#define WIDE_COPY_END }

    for (int t = 0; t < T; ++t) {
        int u0, u1;
        // the conditioning of the live columns, on every member
        for (int s = w; s < nb; s += TNW) {
            const int p = a.seg_pos[b0 + s] + t;
            const bool live = p < a.seg_lim[b0 + s];
            const float *mrow = a.mels_up + (size_t)(live ? p : 0) * M, *arow = a.aux + (size_t)((live ? p : 0) / a.hop) * 4 * A;
            for (int k = lane; k < M; k += 64) in0[(1 + k) * SEG + s] = live ? mrow[k] : 0.f;
            for (int k = lane; k < A; k += 64) {
                in0[(1 + M + k) * SEG + s] = live ? arow[k] : 0.f;          // a1
                va[(H + k) * SEG + s] = live ? arow[A + k] : 0.f;           // a2, behind x1
                vb[(H + k) * SEG + s] = live ? arow[2 * A + k] : 0.f;       // a3, behind x2
            }
        }
        __syncthreads();
        // ---- I: xi -> vb[0..H)
        {
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(0);
            wide_share(H, m, W, u0, u1);
            wide_linear<false>(a.I_T, a.I_b, H, K0, in0, xs, u0, u1, w, lane);
            WIDE_HANDOFF(0)
            WIDE_COPY(xs, H * SEG, i, q)
                *reinterpret_cast<float4 *>(vb + i) = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
            WIDE_COPY_END
            __syncthreads();
        }
        // ---- rnn1 on xi; then h1 <- the new h1 and x1 = xi + h1 -> va[0..H)
        {
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(1);
            wide_gru(a.w_ih1T, a.w_hh1T, a.b_ih1, a.b_hh1, H, H, vb, h1s, xs, u0, u1, w, lane);
            WIDE_HANDOFF(1)
            WIDE_COPY(xs, H * SEG, i, q)
                const float hn[4] = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)};
#pragma unroll
                for (int e = 0; e < 4; ++e) { h1s[i + e] = hn[e]; va[i + e] = vb[i + e] + hn[e]; }
            WIDE_COPY_END
            __syncthreads();
        }
        // ---- rnn2 on [x1 | a2]; then h2 <- the new h2 and x2 = x1 + h2 -> vb[0..H)
        {
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(2);
            wide_gru(a.w_ih2T, a.w_hh2T, a.b_ih2, a.b_hh2, H, H + A, va, h2s, xs, u0, u1, w, lane);
            WIDE_HANDOFF(2)
            WIDE_COPY(xs, H * SEG, i, q)
                const float hn[4] = {__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w)};
#pragma unroll
                for (int e = 0; e < 4; ++e) { h2s[i + e] = hn[e]; vb[i + e] = va[i + e] + hn[e]; }
            WIDE_COPY_END
            __syncthreads();
        }
        // ---- fc1 on [x2 | a3] -> va[0..F), a4 behind it
        {
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(3);
            wide_share(F, m, W, u0, u1);
            wide_linear<true>(a.fc1T, a.fc1_b, F, H + A, vb, xs, u0, u1, w, lane);
            WIDE_HANDOFF(3)     // (every wave has read x1 | a2 of va: the barriers of the hand-off lie in between)
            WIDE_COPY(xs, F * SEG, i, q)
                *reinterpret_cast<float4 *>(va + i) = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
            WIDE_COPY_END
            for (int s = w; s < nb; s += TNW) {             // a4
                const int p = a.seg_pos[b0 + s] + t;
                const bool live = p < a.seg_lim[b0 + s];
                const float *arow = a.aux + (size_t)((live ? p : 0) / a.hop) * 4 * A;
                for (int k = lane; k < A; k += 64) va[(F + k) * SEG + s] = live ? arow[3 * A + k] : 0.f;
            }
            __syncthreads();
        }
        // ---- fc2 on [y1 | a4] -> vb[0..F)
        {
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(4);
            wide_linear<true>(a.fc2T, a.fc2_b, F, F + A, va, xs, u0, u1, w, lane);
            WIDE_HANDOFF(4)
            WIDE_COPY(xs, F * SEG, i, q)
                *reinterpret_cast<float4 *>(vb + i) = make_float4(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w));
            WIDE_COPY_END
            __syncthreads();
        }
        // ---- fc3 and the sampling, per segment
        if (MODE == 1) {                                // every member, wrnn_tile_kernel's code: logits -> red[c][seg]
            for (int tile = w; tile * 16 < C; tile += TNW) {
                f32x4 acc[1];
                tile_dot<1, 32, 1>(a.fc3T, C, 0, tile * 16, F, vb, lane, acc);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = tile * 16 + q4 + v;
                    if (c < C) {
                        const float l = acc[0][v] + a.fc3_b[c];
                        red[c * SEG + seg] = l;
                        if (a.dbg_logits && m == 0 && seg < nb) a.dbg_logits[((size_t)t * B + b0 + seg) * C + c] = l;
                    }
                }
            }
            __syncthreads();
            if (tid < SEG * 16) {                       // 16 lanes per segment, the first ten carry a mixture
                const int s = tid >> 4, mx = tid & 15, b = b0 + s;
                const bool on = s < nb;
                const float *nrow = a.noise + (size_t)t * 11 * B;
                float best = (on && mx < 10) ? mol_gumbel(red[mx * SEG + s], nrow[b * 10 + mx]) : -INFINITY;
                int bidx = mx;
#pragma unroll
                for (int xo = 8; xo >= 1; xo >>= 1) {
                    const float ob = __shfl_xor(best, xo, 16);
                    const int oi = __shfl_xor(bidx, xo, 16);
                    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
                }
                if (on && mx == 0) {
                    float xv = mol_sample(red[(10 + bidx) * SEG + s], red[(20 + bidx) * SEG + s], nrow[10 * B + b]);
                    if (m == 0) a.out[(size_t)b * T + t] = xv;
                    if (a.force_x) xv = a.force_x[(size_t)b * T + t];
                    in0[s] = xv;
                }
            }
        } else {
            // the members' shares of the logits (bias added) -> the stage's buffer as [class][segment]; dbg_logits by the owner of the rows
            const __amdgpu_buffer_rsrc_t xs = WIDE_XS(5);
            wide_share(C, m, W, u0, u1);
            for (int u = u0 + w; u < u1; u += TNW) {
                f32x4 acc[1];
                wide_dot<1, 16>(a.fc3T, C, 0, u * 16, F, vb, lane, acc);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = u * 16 + q4 + v;
                    if (c < C) {
                        const float l = acc[0][v] + a.fc3_b[c];
                        wide_put(xs, c, seg, l);
                        if (a.dbg_logits && seg < nb) a.dbg_logits[((size_t)t * B + b0 + seg) * C + c] = l;
                    }
                }
            }
            WIDE_HANDOFF(5)
            // wrnn_tile_kernel's sampler on the whole vector, in its register layout: lane l holds classes 64 group + 16 (l >> 4) + 4 v + j of segment l & 15
            f32x4 keep[TQ][4];
            const bool on = seg < nb;
            float lmax = -INFINITY;
            // (the wave index as the step's own scalar, and one lane offset per class group formed anew every step: as in wrnn_tile_kernel, so that nothing the
            // unrolled groups derive is hoisted out of the step loop and spilled)
            int ws = __builtin_amdgcn_readfirstlane(w);
            asm volatile("" : "+s"(ws));
            const int cb = ws * 64 + (lane >> 4) * 16;
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
                // class cb + 64 TNW q + 4 v + j at a constant offset; a class past C reads its neighbours or, past the buffer, 0, and is not used
                int voffq = ((cb + q * 64 * TNW) * SEG + seg) * 4;
                asm volatile("" : "+v"(voffq));
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int c = cb + q * 64 * TNW + 4 * v + j;
                        const float l = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xs, voffq + (4 * v + j) * SEG * 4, 0, 16 /* sc1 */));
                        keep[q][j][v] = c < C ? l : -INFINITY;
                        if (c < C) lmax = fmaxf(lmax, l);
                    }
                __builtin_amdgcn_sched_barrier(0);      // (one class group at a time)
            }
            float *rmax = red, *rsum = red + TNW * SEG, *rsum2 = red + 2 * TNW * SEG, *rbst = red + 3 * TNW * SEG;
            int *ridx = reinterpret_cast<int *>(red + 4 * TNW * SEG);
            lmax = fmaxf(lmax, __shfl_xor(lmax, 16, 64));
            lmax = fmaxf(lmax, __shfl_xor(lmax, 32, 64));
            if (lane < SEG) rmax[w * SEG + seg] = lmax;
            __syncthreads();
            float mx = rmax[seg];
#pragma unroll
            for (int ww = 1; ww < TNW; ++ww) mx = fmaxf(mx, rmax[ww * SEG + seg]);
            float part = 0.f;
#pragma unroll
            for (int q = 0; q < TQ; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) { keep[q][j][v] = expf(keep[q][j][v] - mx); part += keep[q][j][v]; }     // (no class: exp(-inf) = 0)
            part += __shfl_xor(part, 16, 64);
            part += __shfl_xor(part, 32, 64);
            if (lane < SEG) rsum[w * SEG + seg] = part;
            __syncthreads();
            float sum = rsum[seg];
#pragma unroll
            for (int ww = 1; ww < TNW; ++ww) sum += rsum[ww * SEG + seg];
            part = 0.f;
#pragma unroll
            for (int q = 0; q < TQ; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) { keep[q][j][v] = keep[q][j][v] / sum; part += keep[q][j][v]; }
            part += __shfl_xor(part, 16, 64);
            part += __shfl_xor(part, 32, 64);
            if (lane < SEG) rsum2[w * SEG + seg] = part;
            __syncthreads();
            float sum2 = rsum2[seg];
#pragma unroll
            for (int ww = 1; ww < TNW; ++ww) sum2 += rsum2[ww * SEG + seg];
            float rbest = -INFINITY;
            int bidx = 0x7FFFFFFF;
            const float *nrow = a.noise + ((size_t)t * B + (on ? b0 + seg : 0)) * C + cb;
            asm volatile("" : "+v"(nrow));
#pragma unroll
            for (int q = 0; q < TQ; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int o = q * 64 * TNW + 4 * v + j;
                        if (on && cb + o < C) {
                            const float rr = (keep[q][j][v] / sum2) / nrow[o];
                            if (rr > rbest) { rbest = rr; bidx = cb + o; }         // ascending class: the first maximum stays
                        }
                    }
#pragma unroll
            for (int xo = 16; xo <= 32; xo <<= 1) {
                const float ob = __shfl_xor(rbest, xo, 64);
                const int oi = __shfl_xor(bidx, xo, 64);
                if (ob > rbest || (ob == rbest && oi < bidx)) { rbest = ob; bidx = oi; }
            }
            if (lane < SEG) { rbst[w * SEG + seg] = rbest; ridx[w * SEG + seg] = bidx; }
            __syncthreads();
            if (tid < nb) {
                float br = rbst[tid];
                int bi = ridx[tid];
                for (int ww = 1; ww < TNW; ++ww) {
                    const float ob = rbst[ww * SEG + tid];
                    const int oi = ridx[ww * SEG + tid];
                    if (ob > br || (ob == br && oi < bi)) { br = ob; bi = oi; }
                }
                float xv = 2.f * (float)bi / ((float)C - 1.f) - 1.f;
                if (m == 0) a.out[(size_t)(b0 + tid) * T + t] = xv;
                if (a.force_x) xv = a.force_x[(size_t)(b0 + tid) * T + t];
                in0[tid] = xv;
            }
        }
        __syncthreads();
        if (a.progress && m == 0) {                     // (uniform) a watched call: the tile's word, by the member that writes `out`
            const int done = t + 1;
            if (done % a.progress_every == 0 || done == T) publish_progress(a.progress + g, (unsigned)done, tid);
        }
    }
#undef WIDE_HANDOFF
#undef WIDE_XS
#undef WIDE_COPY
#undef WIDE_COPY_END
}

// floats per (tile, stage) buffer: the longest stage vector, [rows][16]
static size_t wide_xstride(int H, int F, int C, int mode)
{
    size_t r = (size_t)(H > F ? H : F);
    if (mode != 1 && (size_t)C > r) r = (size_t)C;
    return ((r + 3) & ~(size_t)3) * SEG;
}
// what the workspace holds for `tiles` tiles: the flag block (a multiple of 256 bytes, in front), then the buffers
size_t tile_wide_flag_bytes(int tiles) { return (((size_t)tiles * WIDE_STAGES * WIDE_MAXW * sizeof(unsigned)) + 255) / 256 * 256; }
size_t tile_wide_xbuf_bytes(int tiles, int H, int F, int C, int mode) { return (size_t)tiles * WIDE_STAGES * wide_xstride(H, F, C, mode) * sizeof(float); }

// `xws`: tile_wide_flag_bytes + tile_wide_xbuf_bytes of workspace, 256-byte aligned
hipError_t launch_tile_wide(const GenArgs &args, int mode, int W, void *xws, unsigned *status, hipStream_t stream)
{
    if (W != 2 && W != 4 && W != 8) return hipErrorInvalidValue;
    const int tiles = (args.B + SEG - 1) / SEG;
    const size_t lds = tile_lds_bytes(args.H, args.F, args.M, args.A, args.C);
    const void *fn = mode == 1 ? (const void *)wrnn_tile_wide_kernel<1> : (const void *)wrnn_tile_wide_kernel<0>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // every polled word = 0, which is no epoch: in front of EVERY launch, a block of its own
    if ((e = hipMemsetAsync(xws, 0, tile_wide_flag_bytes(tiles), stream)) != hipSuccess) return e;
    GenArgs a = args;
    WideArgs x;
    x.flags = (unsigned *)xws;
    x.xbuf = (float *)((char *)xws + tile_wide_flag_bytes(tiles));
    x.status = status; x.W = W; x.xstride = (int)wide_xstride(args.H, args.F, args.C, mode);
    void *params[] = {(void *)&a, (void *)&x};
    return hipLaunchCooperativeKernel(fn, dim3(tiles * W), dim3(TNT), params, (unsigned)lds, stream);
}

}  // namespace wrnn
