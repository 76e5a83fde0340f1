// wrnn_tile_sparse.hip -- wrnn_tile_kernel's dataflow for a generic pack whose GRU matrices (and, FCS, fc1 / fc2) are 16x1 block-sparse
// (WRNN_ALGO_TILE_SPARSE, on request).
//
// The kernel IS wrnn_tile_kernel (wrnn_tile.hip: one workgroup per 16 folded segments, activations in LDS as [k][16], segment table, noise, force_x and logits
// handling, the I layer, fc3 and both samplers: wrnn_tile_body.inc) except for the four stages between the I layer and fc3.  Those run on the pack's
// tile-sparse view (TileSparseMat, wrnn_device.h): per block row of 16 consecutive rows the list of the columns that hold a non-zero, so a step streams and
// multiplies the surviving blocks only.
//
//   a tile      one block row = 16 consecutive rows (not wrnn_tile.hip's interleaved 64-row groups: a list belongs to 16 rows)
//   a k-step    four list entries = one v_mfma_f32_16x16x4_f32: lane l supplies A[i = l & 15][k = l >> 4] from the packed values and, as B, the GATHERED
//               activation act[col[4 s + (l >> 4)] * 16 + (l & 15)] (one ds_read_b32)
//   a group     four k-steps = 16 list entries: what a lane fetches with ONE 16-byte load of values and one of columns.  The next group of every list is in
//               flight while the current one is multiplied.  Lists are padded to whole groups (value 0.0f at a valid column); k-steps that hold nothing but
//               padding are not issued
//   GRU stage   a wave owns UNITS: for the 16 units of a tile it runs the r, z, n lists of W_ih and of W_hh -- six lists of different lengths side by side, six
//               accumulators -- and the cell (gru_update) in the D layout, as tile_gru does
//   fc stage    (FCS) a wave runs two tiles side by side; !FCS: tile_linear on the dense k-major copies
// Summation order: an output element is ONE accumulator chain over its block row's list in ascending column order -- it depends on that block row alone, not
// on the wave count nor on what the tile's other segments hold.  A padded entry adds 0.0f * (a finite activation).  An empty block row issues no MFMA: bias.
//
// LDS banks of the gathered B read (ds_read_b32: bank = dword address mod 32, conflicts among the lanes of a 32-lane half): lanes 16 kq + i read dword
// 16 col[kq] + i, i.e. bank 16 (col & 1) + i -- the two k-quads of a half collide (2-way, +1 LDS cycle) exactly when their two columns have the same parity;
// equal columns (padding) broadcast.  The dense kernel reads columns k, k + 1: never.  See DESIGN.md section 3.
#include "wrnn_tile_dev.h"

namespace wrnn {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// N lists side by side: list j = block row `br[j]` of matrix m[j] against the activation vector act[j]; br[j] < 0: no list (out[j] = 0).  Wave-uniform but
// for `lane`.
template <int N>
__device__ __forceinline__ void ts_dot(const TileSparseMat *const (&m)[N], const int (&br)[N], const float *const (&act)[N], int lane, f32x4 (&out)[N])
{
    const int i = lane & 15, kq = lane >> 4;
    const f32x4 *vp[N];
    const i32x4 *cp[N];
    int steps[N], ng[N], maxg = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int g0 = 0, n = 0;
        if (br[j] >= 0) { g0 = m[j]->tab[2 * br[j]]; n = m[j]->tab[2 * br[j] + 1]; }
        steps[j] = (n + 3) >> 2; ng[j] = (n + 15) >> 4;
        vp[j] = reinterpret_cast<const f32x4 *>(m[j]->vals) + (size_t)g0 * 64 + lane;
        cp[j] = reinterpret_cast<const i32x4 *>(m[j]->cols) + (size_t)g0 * 4 + kq;
        maxg = ng[j] > maxg ? ng[j] : maxg;
        out[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 xn[N];
    i32x4 cn[N];
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (ng[j] > 0) { xn[j] = vp[j][0]; cn[j] = cp[j][0]; }
    for (int g = 0; g < maxg; ++g) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (g < ng[j]) {
                const f32x4 x = xn[j];
                const i32x4 c = cn[j];
                if (g + 1 < ng[j]) { xn[j] = vp[j][(size_t)(g + 1) * 64]; cn[j] = cp[j][(size_t)(g + 1) * 4]; }
                const float *bp = act[j] + i;
                const float b0 = bp[c.x * SEG], b1 = bp[c.y * SEG], b2 = bp[c.z * SEG], b3 = bp[c.w * SEG];
                const int left = steps[j] - 4 * g;      // k-steps of this group that hold a surviving column (>= 1)
                out[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b0, out[j], 0, 0, 0);
                if (left > 1) out[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b1, out[j], 0, 0, 0);
                if (left > 2) out[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b2, out[j], 0, 0, 0);
                if (left > 3) out[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b3, out[j], 0, 0, 0);
            }
        }
    }
}

// one GRU stage (H a multiple of 16): tile u = units 16 u .. 16 u + 15 on wave u % TNW; block row g * (H / 16) + u is gate g's.  D: lane l, register v = unit
// 16 u + 4 (l >> 4) + v of segment l & 15
__device__ __forceinline__ void ts_gru(const TileSparseMat &ih, const TileSparseMat &hh, const float *bi, const float *bh, int H, const float *x, const float *hs,
                                       float *dst, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4, nt = H >> 4;
    const int ws = __builtin_amdgcn_readfirstlane(w);
    const TileSparseMat *const m[6] = {&ih, &ih, &ih, &hh, &hh, &hh};
    const float *const act[6] = {x, x, x, hs, hs, hs};
    for (int u = ws; u < nt; u += TNW) {
        const int br[6] = {u, nt + u, 2 * nt + u, u, nt + u, 2 * nt + u};
        f32x4 g[6];
        ts_dot<6>(m, br, act, lane, g);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int un = 16 * u + q4 + v;
            dst[un * SEG + seg] = gru_update(g[0][v] + bi[un], g[1][v] + bi[H + un], g[2][v] + bi[2 * H + un], g[3][v] + bh[un], g[4][v] + bh[H + un],
                                             g[5][v] + bh[2 * H + un], hs[un * SEG + seg]);
        }
    }
}

// one Linear stage with relu (F a multiple of 16): tiles t and t + TNW of a wave side by side
__device__ __forceinline__ void ts_linear(const TileSparseMat &fc, const float *bias, int F, const float *x, float *dst, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4, nt = F >> 4;
    const int ws = __builtin_amdgcn_readfirstlane(w);
    const TileSparseMat *const m[2] = {&fc, &fc};
    const float *const act[2] = {x, x};
    for (int t = ws; t < nt; t += 2 * TNW) {
        const int br[2] = {t, t + TNW < nt ? t + TNW : -1};
        f32x4 y[2];
        ts_dot<2>(m, br, act, lane, y);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (br[j] >= 0) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = 16 * br[j] + q4 + v;
                    dst[r * SEG + seg] = fmaxf(y[j][v] + bias[r], 0.f);
                }
            }
    }
}

// MODE: 0 RAW, 1 MOL (C == 30); FCS: fc1 / fc2 on their lists too
template <int MODE, bool FCS>
__global__ __launch_bounds__(TNT) void wrnn_tile_sparse_kernel(const GenArgs a, const TileSparseArgs sp)
{
#define TILE_STAGE_I(x, dst) tile_linear<false>(a.I_T, a.I_b, H, K0, x, dst, w, lane)
#define TILE_STAGE_RNN1(x, hs, dst) ts_gru(sp.m[0], sp.m[1], a.b_ih1, a.b_hh1, H, x, hs, dst, w, lane)
#define TILE_STAGE_RNN2(x, hs, dst) ts_gru(sp.m[2], sp.m[3], a.b_ih2, a.b_hh2, H, x, hs, dst, w, lane)
#define TILE_STAGE_FC1(x, dst)                                                  \
    do {                                                                        \
        if constexpr (FCS) ts_linear(sp.m[4], a.fc1_b, F, x, dst, w, lane);      \
        else tile_linear<true>(a.fc1T, a.fc1_b, F, H + A, x, dst, w, lane);      \
    } while (0)
#define TILE_STAGE_FC2(x, dst)                                                  \
    do {                                                                        \
        if constexpr (FCS) ts_linear(sp.m[5], a.fc2_b, F, x, dst, w, lane);      \
        else tile_linear<true>(a.fc2T, a.fc2_b, F, F + A, x, dst, w, lane);      \
    } while (0)
#define TILE_FC3_TILE(row0, x, acc) tile_dot<1, 32, 1>(a.fc3T, C, 0, row0, F, x, lane, acc)
#define TILE_FC3_GROUP(row0, x, acc) tile_dot<1, 16, 4>(a.fc3T, C, 0, row0, F, x, lane, acc)
#include "wrnn_tile_body.inc"
#undef TILE_STAGE_I
#undef TILE_FC3_TILE
#undef TILE_FC3_GROUP
#undef TILE_STAGE_RNN1
#undef TILE_STAGE_RNN2
#undef TILE_STAGE_FC1
#undef TILE_STAGE_FC2
}

size_t tile_lds_bytes(int H, int F, int M, int A, int C);

// (the admission rule is wrnn_tile_kernel's: tile_dims_ok / tile_lds_bytes, the activations are the same; the planner has checked it and the view)
hipError_t launch_tile_sparse(const GenArgs &args, const TileSparseArgs &sp, int mode, bool fcs, hipStream_t stream)
{
    const size_t lds = tile_lds_bytes(args.H, args.F, args.M, args.A, args.C);
    const void *fn = mode == 1 ? (fcs ? (const void *)wrnn_tile_sparse_kernel<1, true> : (const void *)wrnn_tile_sparse_kernel<1, false>)
                               : (fcs ? (const void *)wrnn_tile_sparse_kernel<0, true> : (const void *)wrnn_tile_sparse_kernel<0, false>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((args.B + SEG - 1) / SEG);
    if (mode == 1) {
        if (fcs) hipLaunchKernelGGL((wrnn_tile_sparse_kernel<1, true>), grid, dim3(TNT), lds, stream, args, sp);
        else hipLaunchKernelGGL((wrnn_tile_sparse_kernel<1, false>), grid, dim3(TNT), lds, stream, args, sp);
    } else {
        if (fcs) hipLaunchKernelGGL((wrnn_tile_sparse_kernel<0, true>), grid, dim3(TNT), lds, stream, args, sp);
        else hipLaunchKernelGGL((wrnn_tile_sparse_kernel<0, false>), grid, dim3(TNT), lds, stream, args, sp);
    }
    return hipGetLastError();
}

}  // namespace wrnn
