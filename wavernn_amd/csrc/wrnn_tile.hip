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
#include "wrnn_tile_dev.h"

namespace wrnn {

// MODE: 0 RAW, 1 MOL (C == 30)
template <int MODE>
__global__ __launch_bounds__(TNT) void wrnn_tile_kernel(const GenArgs a)
{
#define TILE_STAGE_I(x, dst) tile_linear<false>(a.I_T, a.I_b, H, K0, x, dst, w, lane)
#define TILE_STAGE_RNN1(x, hs, dst) tile_gru(a.w_ih1T, a.w_hh1T, a.b_ih1, a.b_hh1, H, H, x, hs, dst, w, lane)
#define TILE_STAGE_RNN2(x, hs, dst) tile_gru(a.w_ih2T, a.w_hh2T, a.b_ih2, a.b_hh2, H, H + A, x, hs, dst, w, lane)
#define TILE_STAGE_FC1(x, dst) tile_linear<true>(a.fc1T, a.fc1_b, F, H + A, x, dst, w, lane)
#define TILE_STAGE_FC2(x, dst) tile_linear<true>(a.fc2T, a.fc2_b, F, F + A, x, dst, w, lane)
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
