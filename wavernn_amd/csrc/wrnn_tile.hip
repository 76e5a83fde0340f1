// wrnn_tile.hip -- the dimension-generic loop kernel for a TILE of up to 16 folded segments per workgroup (WRNN_ALGO_TILE, on request).
//
// The dataflow is wrnn_generic_kernel's (wrnn_generic.hip: fatchord_version.py:203-237 verbatim, nothing hoisted) and so is the pack: the k-major copies
// XT[k][rows] of GenArgs.  What changes is who shares a read of the weights: workgroup g owns segments [16 g, min(16 g + 16, B)) and every matrix product
// is a chain of v_mfma_f32_16x16x4_f32 whose N dimension is those 16 segments, so a step streams the weights once per 16 segments instead of once per
// segment.  No workgroup ever waits for another: no exchange, no polling, no cooperative launch.
//
//   A operand   a wave works on a GROUP of 64 consecutive rows as four 16-row tiles with the rows interleaved: tile j holds rows row0 + 4 i + j, i = 0..15.
//               Lane l reads ONE 16-byte word per k, XT[(k0 + (l >> 4)) * ld + row0 + 4 (l & 15) .. + 3], and its four floats are the A operands
//               A[i = l & 15][k = l >> 4] of the four tiles' MFMAs.  (Measured: with one dword per lane -- sixteen consecutive rows per tile -- a workgroup
//               streams its weights at 35 GB/s, the rate of wrnn_generic_kernel's loads: a CU's vector-memory path takes four lanes per clock whatever
//               their width.)  MoL's fc3 (30 rows) keeps the one-dword form, tile = sixteen consecutive rows, on two waves.
//               Rows past the matrix's row count read their neighbours' weights -- a row of A touches that row of D only, and it is never written --;
//               the K tail (K no multiple of 4) supplies 0.
//   B operand   activations live in LDS as [k][16 segments]: lane l reads act[(k0 + (l >> 4)) * 16 + (l & 15)] (one ds_read_b32, conflict-free).
//   D           lane l, register v = tile row 4 (l >> 4) + v, i.e. row row0 + 16 (l >> 4) + 4 v + j of the group; segment l & 15.
// A wave takes whole groups and runs the whole K of a group itself, its operands prefetched through a register ring (tile_dot): there are no cross-wave
// partial sums, and an output element is ONE chain of MFMAs in ascending k -- its summation order depends on K alone, neither on the wave count nor on
// what the tile's other columns hold.  (The four, or twelve, independent chains of a group hide the 40-cycle dependent-accumulator latency behind the
// 32-cycle issue; the one-dword form alternates two accumulators instead, as mfma_tile of wrnn_device.h does.)  Dead columns of the last tile compute
// on zeros and write nothing.
//
// LDS (floats, every vector as [k][16]):  in0[K0] | va[HF] | vb[HF] | h1s[H] | h2s[H] | red[TRED],  K0 = 1 + M + A, HF = max(H, F) + A, row counts
// rounded up to 4.  A GRU stage writes the new h into the ping-pong vector that is free at that point (rnn1: va, rnn2: vb) and a pointwise pass moves
// it behind a barrier, once every wave has read the old one.
#include "wrnn_device.h"

namespace wrnn {

constexpr int TNT = 512;                // threads per workgroup: one workgroup per CU (its LDS), two waves per SIMD, <= 256 VGPRs
constexpr int TNW = TNT / 64;           // 8 waves; wave w also loads the conditioning of the tile's segments w and w + 8
constexpr int TQ = 4;                   // RAW: 64-class groups a wave keeps in registers through the sampler: C <= TQ * TNW * 64 = 2048
constexpr int TRED = 5 * TNW * SEG;     // sampler scratch: RAW five [wave][segment] reduction planes; MOL the logits [30][16]
constexpr size_t TILE_LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ int r4(int n) { return (n + 3) & ~3; }

// NG row groups of one k-major matrix against one activation vector over k in [0, K); group g starts at row row0 + g * gstride.
// V = 4: a group is 64 rows = four interleaved tiles, out[4 g + j] = rows row0 + g * gstride + 4 i + j; one 16-byte load per lane and k-step; one accumulator
// per tile.  V = 1: a group is one tile of 16 consecutive rows, one dword per lane; k-step j goes to accumulator j & 1.
// The operands of the next D k-steps (D even) ride in a register ring: slot j % D is refilled with step j + D as soon as step j's MFMAs are issued, so
// D * NG loads are in flight per wave for the whole dot product.  They are buffer loads: one lane offset per group, the step in the scalar offset, no
// address arithmetic in the loop; the resource ends with the matrix, so a read past it (rows past the row count, at the last k) returns 0.
template <int NG, int D, int V>
__device__ __forceinline__ void tile_dot(const float *WT, int ld, int gstride, int row0, int K, const float *act, int lane, f32x4 (&out)[NG * V])
{
    static_assert(D % 2 == 0 && (V == 1 || V == 4), "tile_dot: whole pairs of k-steps; one or four floats per lane");
    constexpr int NACC = V == 1 ? 2 : 1, NM = NG * V;
    const int i = lane & 15, kq = lane >> 4;
    const float *bp = act + kq * SEG + i;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(WT, (unsigned)K * (unsigned)ld * 4u);
    int voff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) voff[g] = (kq * ld + row0 + V * i + g * gstride) * 4;
    const int nfull = K >> 2, sstep = 16 * ld;                  // whole k-steps; bytes from one k-step to the next
    float x[D][NM], bv[D];
    f32x4 acc[NACC][NM];
#pragma unroll
    for (int n = 0; n < NACC; ++n)
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[n][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](float (&dst)[NM], int off0, int soff) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if constexpr (V == 4) {
                const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, off0 + g * gstride * 4, soff, 0);
                dst[4 * g + 0] = __uint_as_float(r.x); dst[4 * g + 1] = __uint_as_float(r.y);
                dst[4 * g + 2] = __uint_as_float(r.z); dst[4 * g + 3] = __uint_as_float(r.w);
            } else dst[g] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off0 + g * gstride * 4, soff, 0));
        }
    };
    auto fill = [&](int d, int j) { load(x[d], voff[0], j * sstep); bv[d] = bp[j * 4 * SEG]; };
    auto use = [&](int d) {
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[d % NACC][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[d][m], bv[d], acc[d % NACC][m], 0, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nfull) fill(d, d);
    int j0 = 0;
    for (; j0 + 2 * D <= nfull; j0 += D) {          // every step of the group exists, and so does its successor in the ring
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
    // the K tail (K no multiple of 4): k >= K supplies 0, read from a clamped address; the activation rows up to the next multiple of 4 exist
    if (K & 3) {
        const int k = 4 * nfull + kq;
        const float b = bp[nfull * 4 * SEG];
        float xt[NM];
        load(xt, ((k < K ? k : K - 1) * ld + row0 + V * i) * 4, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float xv = k < K ? xt[m] : 0.f;
            if (NACC == 2 && (nfull & 1)) acc[NACC - 1][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, b, acc[NACC - 1][m], 0, 0, 0);
            else acc[0][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, b, acc[0][m], 0, 0, 0);
        }
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) out[m] = NACC == 2 ? acc[0][m] + acc[NACC - 1][m] : acc[0][m];
}

// one Linear stage: dst[r][seg] = [relu](XT . act + bias), rows r < R, in groups of 64 rows
template <bool RELU>
__device__ __forceinline__ void tile_linear(const float *WT, const float *bias, int R, int K, const float *act, float *dst, int w, int lane)
{
    const int seg = lane & 15, q16 = (lane >> 4) * 16;
    for (int grp = w; grp * 64 < R; grp += TNW) {
        f32x4 acc[4];
        tile_dot<1, 16, 4>(WT, R, 0, grp * 64, K, act, lane, acc);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = grp * 64 + q16 + 4 * v + j;
                if (r < R) { const float y = acc[j][v] + bias[r]; dst[r * SEG + seg] = RELU ? fmaxf(y, 0.f) : y; }
            }
    }
}

// one GRU stage: the six gate groups of 64 units on one wave, the cell in the D layout; the new h goes to `dst` (the old one is still being read)
__device__ __forceinline__ void tile_gru(const float *WiT, const float *WhT, const float *bi, const float *bh, int H, int K1, const float *x, const float *hs,
                                         float *dst, int w, int lane)
{
    const int seg = lane & 15, q16 = (lane >> 4) * 16;
    for (int grp = w; grp * 64 < H; grp += TNW) {
        f32x4 gi[12], gh[12];
        tile_dot<3, 6, 4>(WiT, 3 * H, H, grp * 64, K1, x, lane, gi);
        tile_dot<3, 6, 4>(WhT, 3 * H, H, grp * 64, H, hs, lane, gh);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = grp * 64 + q16 + 4 * v + j;
                if (u < H)
                    dst[u * SEG + seg] = gru_update(gi[j][v] + bi[u], gi[4 + j][v] + bi[H + u], gi[8 + j][v] + bi[2 * H + u], gh[j][v] + bh[u],
                                                    gh[4 + j][v] + bh[H + u], gh[8 + j][v] + bh[2 * H + u], hs[u * SEG + seg]);
            }
    }
}

// MODE: 0 RAW, 1 MOL (C == 30)
template <int MODE>
__global__ __launch_bounds__(TNT) void wrnn_tile_kernel(const GenArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float tsm[];
    const int H = a.H, F = a.F, M = a.M, A = a.A, C = a.C, T = a.T, B = a.B;
    const int K0 = 1 + M + A, HF = (H > F ? H : F) + A;
    float *in0 = tsm, *va = in0 + r4(K0) * SEG, *vb = va + r4(HF) * SEG, *h1s = vb + r4(HF) * SEG, *h2s = h1s + r4(H) * SEG, *red = h2s + r4(H) * SEG;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, seg = lane & 15, q4 = (lane >> 4) * 4;
    const int b0 = blockIdx.x * SEG, nb = (B - b0 < SEG) ? B - b0 : SEG;
    // h1 = h2 = 0, x_{-1} = 0 (fatchord_version.py:194-196); the padding rows and the dead columns stay 0 for the whole run
    for (int i = tid; i < (int)(red - tsm) + TRED; i += TNT) tsm[i] = 0.f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        // the conditioning of the live columns: wave w loads segments w, w + TNW, ... (a dead column keeps its zeros)
        for (int s = w; s < nb; s += TNW) {
            const int p = a.seg_pos[b0 + s] + t;
            const bool live = p < a.seg_lim[b0 + s];    // past the utterance: the fold's zero padding (:326-330)
            const float *mrow = a.mels_up + (size_t)(live ? p : 0) * M, *arow = a.aux + (size_t)((live ? p : 0) / a.hop) * 4 * A;
            for (int k = lane; k < M; k += 64) in0[(1 + k) * SEG + s] = live ? mrow[k] : 0.f;
            for (int k = lane; k < A; k += 64) {
                in0[(1 + M + k) * SEG + s] = live ? arow[k] : 0.f;          // a1
                va[(H + k) * SEG + s] = live ? arow[A + k] : 0.f;           // a2, behind x1
                vb[(H + k) * SEG + s] = live ? arow[2 * A + k] : 0.f;       // a3, behind x2 (neither I nor the GRU stages touch these rows)
            }
        }
        __syncthreads();
        // ---- I (:208-209): xi -> vb[0..H)
        tile_linear<false>(a.I_T, a.I_b, H, K0, in0, vb, w, lane);
        __syncthreads();
        // ---- rnn1 (:210) on xi; the new h1 -> va[0..H), then h1 <- it and x1 = xi + h1 (:212) -> va[0..H)
        tile_gru(a.w_ih1T, a.w_hh1T, a.b_ih1, a.b_hh1, H, H, vb, h1s, va, w, lane);
        __syncthreads();                                // every wave has read the old h1
        for (int i = tid; i < H * SEG; i += TNT) { const float hn = va[i]; h1s[i] = hn; va[i] = vb[i] + hn; }
        __syncthreads();
        // ---- rnn2 (:213-214) on [x1 | a2]; the new h2 -> vb[0..H) (xi is dead), then h2 <- it and x2 = x1 + h2 (:216) -> vb[0..H)
        tile_gru(a.w_ih2T, a.w_hh2T, a.b_ih2, a.b_hh2, H, H + A, va, h2s, vb, w, lane);
        __syncthreads();
        for (int i = tid; i < H * SEG; i += TNT) { const float hn = vb[i]; h2s[i] = hn; vb[i] = va[i] + hn; }
        __syncthreads();
        // ---- fc1 (:217-218) on [x2 | a3] -> va[0..F), a4 behind it (va is free: x1 | a2 were last read above)
        tile_linear<true>(a.fc1T, a.fc1_b, F, H + A, vb, va, w, lane);
        for (int s = w; s < nb; s += TNW) {             // a4
            const int p = a.seg_pos[b0 + s] + t;
            const bool live = p < a.seg_lim[b0 + s];
            const float *arow = a.aux + (size_t)((live ? p : 0) / a.hop) * 4 * A;
            for (int k = lane; k < A; k += 64) va[(F + k) * SEG + s] = live ? arow[3 * A + k] : 0.f;
        }
        __syncthreads();
        // ---- fc2 (:220-221) on [y1 | a4] -> vb[0..F)
        tile_linear<true>(a.fc2T, a.fc2_b, F, F + A, va, vb, w, lane);
        __syncthreads();
        // ---- fc3 (:223) and the sampling, per segment
        if (MODE == 1) {                                // utils/distribution.py:102-121 (C = 30: 10 mixtures); logits -> red[c][seg]
            for (int tile = w; tile * 16 < C; tile += TNW) {
                f32x4 acc[1];
                tile_dot<1, 32, 1>(a.fc3T, C, 0, tile * 16, F, vb, lane, acc);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int c = tile * 16 + q4 + v;
                    if (c < C) {
                        const float l = acc[0][v] + a.fc3_b[c];
                        red[c * SEG + seg] = l;
                        if (a.dbg_logits && seg < nb) a.dbg_logits[((size_t)t * B + b0 + seg) * C + c] = l;
                    }
                }
            }
            __syncthreads();
            if (tid < SEG * 16) {                       // 16 lanes per segment, the first ten carry a mixture
                const int s = tid >> 4, m = tid & 15, b = b0 + s;
                const bool on = s < nb;
                const float *nrow = a.noise + (size_t)t * 11 * B;
                float best = (on && m < 10) ? mol_gumbel(red[m * SEG + s], nrow[b * 10 + m]) : -INFINITY;
                int bidx = m;
#pragma unroll
                for (int x = 8; x >= 1; x >>= 1) {
                    const float ob = __shfl_xor(best, x, 16);
                    const int oi = __shfl_xor(bidx, x, 16);
                    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
                }
                if (on && m == 0) {
                    float x = mol_sample(red[(10 + bidx) * SEG + s], red[(20 + bidx) * SEG + s], nrow[10 * B + b]);
                    a.out[(size_t)b * T + t] = x;
                    if (a.force_x) x = a.force_x[(size_t)b * T + t];
                    in0[s] = x;
                }
            }
        } else {                                        // :232-237 softmax -> Categorical renormalisation -> argmax(p / q), first max wins
            // the logits of a wave's class groups stay in its registers: lane l holds classes 64 group + 16 (l >> 4) + 4 v + j of segment l & 15
            f32x4 keep[TQ][4];
            const bool on = seg < nb;
            float lmax = -INFINITY;
            // (the wave index as the step's own scalar: hoisted out of the step loop, what the unrolled class groups derive from it spills)
            int ws = __builtin_amdgcn_readfirstlane(w);
            asm volatile("" : "+s"(ws));
            // (class cb + 64 TNW q + 4 v + j: bias, noise and logits are read and written at constant offsets from ONE pointer each, formed anew every step)
            const int cb = ws * 64 + (lane >> 4) * 16;
            const float *fb = a.fc3_b + cb;
            float *dl = (a.dbg_logits && on) ? a.dbg_logits + ((size_t)t * B + b0 + seg) * C + cb : nullptr;
            asm volatile("" : "+v"(fb), "+v"(dl));
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
                const int grp = ws + q * TNW;
#pragma unroll
                for (int j = 0; j < 4; ++j) keep[q][j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (grp * 64 < C) {
                    f32x4 acc[4];
                    tile_dot<1, 16, 4>(a.fc3T, C, 0, grp * 64, F, vb, lane, acc);
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int o = q * 64 * TNW + 4 * v + j;
                            if (cb + o < C) {
                                const float l = acc[j][v] + fb[o];
                                keep[q][j][v] = l;
                                lmax = fmaxf(lmax, l);
                                if (dl) dl[o] = l;
                            }
                        }
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
            for (int x = 16; x <= 32; x <<= 1) {
                const float ob = __shfl_xor(rbest, x, 64);
                const int oi = __shfl_xor(bidx, x, 64);
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
                float x = 2.f * (float)bi / ((float)C - 1.f) - 1.f;
                a.out[(size_t)(b0 + tid) * T + t] = x;
                if (a.force_x) x = a.force_x[(size_t)(b0 + tid) * T + t];
                in0[tid] = x;
            }
        }
        __syncthreads();
    }
}

size_t tile_lds_bytes(int H, int F, int M, int A, int C)
{
    (void)C;            // (RAW logits stay in registers, MOL's 30 live in the sampler scratch)
    const size_t K0 = 1 + (size_t)M + A, HF = (size_t)(H > F ? H : F) + A;
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    return ((up4(K0) + 2 * up4(HF) + 2 * up4((size_t)H)) * SEG + TRED) * sizeof(float);
}

// dims this kernel can take: its LDS carve fits one CU's 160 KiB, and a wave can keep its share of the RAW classes
bool tile_dims_ok(int H, int F, int M, int A, int C, int mode)
{
    if (H < 1 || F < 1 || M < 1 || A < 1 || H > 8192 || F > 8192 || M + A > 8192) return false;
    if (mode == 1 ? C != 30 : (C < 2 || C > TQ * TNW * 64)) return false;
    return tile_lds_bytes(H, F, M, A, C) <= TILE_LDS_LIMIT;
}

hipError_t launch_tile(const GenArgs &args, int mode, hipStream_t stream)
{
    const size_t lds = tile_lds_bytes(args.H, args.F, args.M, args.A, args.C);
    const void *fn = mode == 1 ? (const void *)wrnn_tile_kernel<1> : (const void *)wrnn_tile_kernel<0>;
    // (more than 64 KB of dynamic LDS has to be asked for)
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((args.B + SEG - 1) / SEG);
    if (mode == 1) hipLaunchKernelGGL(wrnn_tile_kernel<1>, grid, dim3(TNT), lds, stream, args);
    else hipLaunchKernelGGL(wrnn_tile_kernel<0>, grid, dim3(TNT), lds, stream, args);
    return hipGetLastError();
}

}  // namespace wrnn
