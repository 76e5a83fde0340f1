// wrnn_tile_dev.h -- device functions of the 16-segment tile dataflow, shared by wrnn_tile_kernel (wrnn_tile.hip, whose header describes the operand layouts
// and the LDS carve) and wrnn_tile_sparse_kernel (wrnn_tile_sparse.hip): the MFMA dot product over a k-major matrix and the dense Linear and GRU stages.  The
// body of the kernels is wrnn_tile_body.inc.
#pragma once
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

}  // namespace wrnn
