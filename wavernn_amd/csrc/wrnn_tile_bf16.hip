// wrnn_tile_bf16.hip -- wrnn_tile_kernel's dataflow with the eight loop matrices stored as bfloat16 and multiplied on v_mfma_f32_16x16x32_bf16
// (WRNN_ALGO_TILE_BF16, on request).  NOT the reference's arithmetic: the weights are rounded.
//
// The kernel IS wrnn_tile_kernel (wrnn_tile.hip: one workgroup per 16 folded segments, no exchange, the activations of the 16 segments in LDS as float32
// [k][16], segment table, conditioning, noise, force_x and logits handling, both samplers: wrnn_tile_body.inc) except for its eight matrix products.
//
// THE ARITHMETIC.  Only the weights lose precision: wrnn_pack_create rounds the eight matrices once, on the host, to bfloat16, round-to-nearest-even
// (bf16_round_state_dict of wavernn_amd/synthetic.py does the same in numpy); biases, activations, the GRU state and every pointwise pass stay float32.
// Where an activation x becomes the B operand of an MFMA it is split in registers into three bf16 pieces by truncation,
//     hi = x & 0xFFFF0000,  mid = (x - hi) & 0xFFFF0000,  lo = x - hi - mid
// -- each takes the next 8 bits of the 24-bit significand, so hi + mid + lo == x exactly and every piece is a bf16 number (below about 2^-100 the low pieces
// may flush to zero) --, and an 8-bit x 8-bit product is exact in float32: the kernel computes float32 sums of EXACT products on the rounded weights, the
// quantity a float32 kernel computes on those weights up to the summation order and the MFMA's internal adder.
// An output element is ONE accumulator chain in a fixed order: k-steps of 32 ascending, inside a step the hi, the mid, then the lo MFMA.  There are no
// cross-wave partial sums: a segment's samples depend on neither the wave count nor on what the tile's other columns hold.
//
// THE IMAGE of one matrix W [R rows][K] (tile_bf16_pack of wrnn_abi.hip; wrnn_debug_tile_bf16_pack packs one on the host alone):
//     bf16 img[s = k / 32][row][kq = k % 4][j = (k % 32) / 4],   ceil(K / 32) k-steps, 64 bytes per row and k-step, k >= K: +0; no padding between the
//     rows or the k-steps, 64 rows of +0 (4096 bytes) behind the last k-step
//   A operand   lane l reads ONE 16-byte word per tile and k-step, img[s][row][l >> 4][0..7]: its eight values are A[i = l & 15][8 (l >> 4) + j] of one
//               v_mfma_f32_16x16x32_bf16, which here carry k = 32 s + 4 j + (l >> 4).  (The MFMA sums over its 32 k: which k sits in which slot is free
//               as long as A and B agree.  This assignment keeps the B reads those of wrnn_tile_kernel: the four k-quads of a wave read consecutive
//               rows of the [k][16] vector, 64 consecutive dwords, conflict-free; with k = 8 (l >> 4) + j they would be 128 dwords apart, 2-way.)
//               A wave works on a GROUP of 64 rows as four tiles.  In the I, GRU and fc1 / fc2 stages tile t holds the CONSECUTIVE rows row0 + 16 t + i:
//               one load instruction reads 1024 contiguous bytes.  (Measured with wrnn_tile_kernel's interleaved tiles, rows row0 + 4 i + t, where an
//               instruction reads sixteen 64-byte pieces 256 bytes apart and every 128-byte line is asked for twice: 276 us per step instead of
//               178 for 10-bit rnn = fc = 512, 256 segments.)  fc3 keeps wrnn_tile_kernel's row ownership, which the samplers of the shared body read: RAW the
//               interleaved tiles (IL), MoL one tile of 16 consecutive rows.
//               A row past R (a group's rows may reach 63 past it) reads the next k-step's rows, at the last k-step
//               the zeros behind it: finite weights into a row of D that is never written, and every address a lane forms lies inside the image.  They
//               are buffer loads all the same (one lane offset, the k-step in the scalar offset): the resource ends with the image, past it reads 0.
//   B operand   lane l reads act[(32 s + 4 j + (l >> 4)) * 16 + (l & 15)], j = 0..7 (eight ds_read_b32, as many per 32 k as wrnn_tile_kernel issues)
//               and splits them.  The K tail (K no multiple of 32): k >= K supplies 0.0f from a clamped address -- a zero weight never meets a stale or
//               non-finite LDS word.
//   D           as v_mfma_f32_16x16x4_f32: lane l, register v = tile row 4 (l >> 4) + v, segment l & 15.
// The operands of the next k-steps ride in a register ring (bf_dot): two k-steps in the GRU and Linear stages (24 KiB in flight per wave in a GRU stage; six
// k-steps in a Linear stage measured 4 % slower at rnn = fc = 256), four in RAW's fc3 (whose logits stay in registers beside it), eight in MoL's.
//
// THE LDS RULE is wrnn_tile_kernel's (tile_lds_bytes / tile_dims_ok, row counts rounded up to 4; the vectors keep their layout):
// 16 * 4 * (up4(1 + feat + aux) + 2 * up4(max(rnn, fc) + aux) + 2 * up4(rnn)) + 2560 bytes <= 163840; RAW: <= 2048 classes.
#include "wrnn_tile_dev.h"

namespace wrnn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// NG row groups of one bf16 image against one activation vector over k in [0, K), ADDED to the accumulators the caller hands in; group g starts at row
// row0 + g * gstride.  V = 4: a group is four tiles, tile t = rows row0 + g * gstride + 16 t + i (IL: interleaved, + 4 i + t); V = 1: one tile of 16 rows.  One
// accumulator per tile: acc[V g + t], the LAST group's SKIP groups further on (bf_gru).  The operands of the next D k-steps ride in a register ring: slot
// s % D is refilled with step s + D as soon as step s's MFMAs are issued, so D * NG * V 16-byte loads are in flight per wave for the whole dot product.
template <int NG, int V, int D, int SKIP = 0, bool IL = false, int NA>
__device__ __forceinline__ void bf_dot(const uint16_t *img, int R, int gstride, int row0, int K, const float *act, int lane, f32x4 (&acc)[NA])
{
    static_assert(V == 1 || V == 4, "bf_dot: one tile or four tiles per group");
    static_assert(NA >= (NG + SKIP) * V, "bf_dot: an accumulator per tile");
    constexpr int NM = NG * V;
    auto out = [&](int m) -> f32x4 & { return acc[m < (NG - 1) * V ? m : m + SKIP * V]; };
    // (the lane's offsets are formed anew in every call: hoisted out of the step loop for every call site at once, they spill)
    asm volatile("" : "+v"(lane));
    const int i = lane & 15, kq = lane >> 4;
    const int nsteps = (K + 31) >> 5, nfull = K >> 5;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(img, ((unsigned)nsteps * (unsigned)R + 64u) * 64u);
    const int voff = (row0 + (IL ? V * i : i)) * 64 + kq * 16, sstep = R * 64;    // bytes from one k-step to the next
    const float *bp = act + kq * SEG + i;
    u32x4 x[D][NM];
    float bv[D][8];
    auto fill = [&](int d, int s) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int t = 0; t < V; ++t) x[d][V * g + t] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + (g * gstride + (IL ? t : 16 * t)) * 64, s * sstep, 0);
        if (s < nfull) {
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[d][j] = bp[(32 * s + 4 * j) * SEG];
        } else {                                    // the K tail
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * s + 4 * j + kq;
                const float v = act[(k < K ? k : K - 1) * SEG + i];
                bv[d][j] = k < K ? v : 0.f;
            }
        }
    };
    auto use = [&](int d) {
        u32x4 hi, mid, lo;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float a = bv[d][2 * p], b = bv[d][2 * p + 1];
            const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
            const float ra = a - __uint_as_float(ua & 0xFFFF0000u), rb = b - __uint_as_float(ub & 0xFFFF0000u);
            const unsigned uma = __float_as_uint(ra), umb = __float_as_uint(rb);
            const float la = ra - __uint_as_float(uma & 0xFFFF0000u), lb = rb - __uint_as_float(umb & 0xFFFF0000u);
            // (the upper halves of two words side by side: element 2 p in the low half)
            hi[p] = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
            mid[p] = __builtin_amdgcn_perm(umb, uma, 0x07060302u);
            lo[p] = __builtin_amdgcn_perm(__float_as_uint(lb), __float_as_uint(la), 0x07060302u);
        }
        const bf16x8 bh = __builtin_bit_cast(bf16x8, hi), bm = __builtin_bit_cast(bf16x8, mid), bl = __builtin_bit_cast(bf16x8, lo);
#pragma unroll
        for (int m = 0; m < NM; ++m) out(m) = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x[d][m]), bh, out(m), 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) out(m) = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x[d][m]), bm, out(m), 0, 0, 0);
#pragma unroll
        for (int m = 0; m < NM; ++m) out(m) = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, x[d][m]), bl, out(m), 0, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nsteps) fill(d, d);
    for (int s = 0; s < nsteps; s += D) {
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (s + d < nsteps) {
                use(d);
                if (s + d + D < nsteps) fill(d, s + d + D);
            }
    }
}

// one Linear stage: dst[r][seg] = [relu](W . act + bias), rows r < R, in groups of 64 rows; acc[t][v] of lane l = row 64 grp + 16 t + 4 (l >> 4) + v
template <bool RELU>
__device__ __forceinline__ void bf_linear(const uint16_t *img, const float *bias, int R, int K, const float *act, float *dst, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4;
    for (int grp = w; grp * 64 < R; grp += TNW) {
        f32x4 acc[4] = {};
        bf_dot<1, 4, 2>(img, R, 0, grp * 64, K, act, lane, acc);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = grp * 64 + 16 * j + q4 + v;
                if (r < R) { const float y = acc[j][v] + bias[r]; dst[r * SEG + seg] = RELU ? fmaxf(y, 0.f) : y; }
            }
    }
}

// one GRU stage: the gate groups of 64 units on one wave, the cell in the D layout (rows as in bf_linear); the new h goes to `dst`.  The cell reads gi_r + gh_r and
// gi_z + gh_z only as sums, so r and z are ONE chain each over W_ih's k-steps, then W_hh's (twelve accumulator tiles fewer in registers); gi_n and gh_n,
// which the cell needs apart, keep a chain each: g = r | z | gi_n | gh_n
__device__ __forceinline__ void bf_gru(const uint16_t *Wi, const uint16_t *Wh, const float *bi, const float *bh, int H, int K1, const float *x, const float *hs,
                                       float *dst, int w, int lane)
{
    const int seg = lane & 15, q4 = (lane >> 4) * 4;
    for (int grp = w; grp * 64 < H; grp += TNW) {
        f32x4 g[16] = {};
        bf_dot<3, 4, 2>(Wi, 3 * H, H, grp * 64, K1, x, lane, g);          // r, z, gi_n
        bf_dot<3, 4, 2, 1>(Wh, 3 * H, H, grp * 64, H, hs, lane, g);       // r, z, gh_n
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = grp * 64 + 16 * j + q4 + v;
                if (u < H)
                    dst[u * SEG + seg] = gru_update(g[j][v] + bi[u], g[4 + j][v] + bi[H + u], g[8 + j][v] + bi[2 * H + u], bh[u], bh[H + u],
                                                    g[12 + j][v] + bh[2 * H + u], hs[u * SEG + seg]);
            }
    }
}

// MODE: 0 RAW, 1 MOL (C == 30)
template <int MODE>
__global__ __launch_bounds__(TNT) void wrnn_tile_bf16_kernel(const GenArgs a, const TileBf16Args bw)
{
#define TILE_STAGE_I(x, dst) bf_linear<false>(bw.m[0], a.I_b, H, K0, x, dst, w, lane)
#define TILE_STAGE_RNN1(x, hs, dst) bf_gru(bw.m[1], bw.m[2], a.b_ih1, a.b_hh1, H, H, x, hs, dst, w, lane)
#define TILE_STAGE_RNN2(x, hs, dst) bf_gru(bw.m[3], bw.m[4], a.b_ih2, a.b_hh2, H, H + A, x, hs, dst, w, lane)
#define TILE_STAGE_FC1(x, dst) bf_linear<true>(bw.m[5], a.fc1_b, F, H + A, x, dst, w, lane)
#define TILE_STAGE_FC2(x, dst) bf_linear<true>(bw.m[6], a.fc2_b, F, F + A, x, dst, w, lane)
#define TILE_FC3_TILE(row0, x, acc) do { acc[0] = f32x4{0.f, 0.f, 0.f, 0.f}; bf_dot<1, 1, 8>(bw.m[7], C, 0, row0, F, x, lane, acc); } while (0)
#define TILE_FC3_GROUP(row0, x, acc)                                                    \
    do {                                                                                \
        acc[0] = acc[1] = acc[2] = acc[3] = f32x4{0.f, 0.f, 0.f, 0.f};                  \
        bf_dot<1, 4, 4, 0, true>(bw.m[7], C, 0, row0, F, x, lane, acc);                            \
    } while (0)
#include "wrnn_tile_body.inc"
#undef TILE_STAGE_I
#undef TILE_STAGE_RNN1
#undef TILE_STAGE_RNN2
#undef TILE_STAGE_FC1
#undef TILE_STAGE_FC2
#undef TILE_FC3_TILE
#undef TILE_FC3_GROUP
}

size_t tile_lds_bytes(int H, int F, int M, int A, int C);

// (the admission rule is wrnn_tile_kernel's: the planner has checked it and that the pack has its bf16 view)
hipError_t launch_tile_bf16(const GenArgs &args, const TileBf16Args &bw, int mode, hipStream_t stream)
{
    const size_t lds = tile_lds_bytes(args.H, args.F, args.M, args.A, args.C);
    const void *fn = mode == 1 ? (const void *)wrnn_tile_bf16_kernel<1> : (const void *)wrnn_tile_bf16_kernel<0>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const dim3 grid((args.B + SEG - 1) / SEG);
    if (mode == 1) hipLaunchKernelGGL(wrnn_tile_bf16_kernel<1>, grid, dim3(TNT), lds, stream, args, bw);
    else hipLaunchKernelGGL(wrnn_tile_bf16_kernel<0>, grid, dim3(TNT), lds, stream, args, bw);
    return hipGetLastError();
}

}  // namespace wrnn
