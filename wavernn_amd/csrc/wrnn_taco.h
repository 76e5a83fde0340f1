// wrnn_taco.h -- what the Tacotron decoder kernels share (wrnn_taco.hip: one sentence per launch; wrnn_taco_batch.hip: up to eight): the
// decoder's geometry, the workspace prefix that holds the status words, and the row arithmetic -- one definition, so that the batched kernel
// sums in exactly the order of the single-sentence one.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wavernn_amd.h"
#include "wrnn_device.h"

// host side (wrnn_taco.hip): the message behind wrnn_taco_last_error(), and the one check of the geometry every decoder kernel is built for
// (T_NM .. T_AK below): WRNN_OK, or WRNN_ERR_ARG with the message behind `pre` ("" or "group g: ")
void taco_err(const char *fmt, ...);
int taco_check_geometry(const wrnn_taco_weights *w, const char *pre);

namespace wrnn {

constexpr int T_NM = 80;        // mel channels
constexpr int T_P1 = 256;       // prenet fc1
constexpr int T_P2 = 128;       // prenet fc2
constexpr int T_DD = 256;       // decoder dims (attention GRU hidden) == encoder sequence width (context)
constexpr int T_LD = 512;       // LSTM dims
constexpr int T_AF = 32;        // attention location filters
constexpr int T_AK = 31;        // ... their taps
constexpr int T_NMAX = 1024;    // encoder positions the workspace is laid out for
constexpr int T_MAXWG = 128;

// workspace (floats)
constexpr int A_PRE_IN = 0, A_PRE1 = 128, A_PRE2 = 384, A_ATTN_H = 512 /* [2][256] */, A_CTX = 1024, A_PQ = 1280,
              A_S = 1536 /* [NMAX] */, A_CUM = 2560, A_ATT = 3584, A_X = 4608, A_X2 = 5120, A_X3 = 5632,
              A_H1 = 6144 /* [2][512] */, A_H2 = 7168, A_C1 = 8192, A_C2 = 8704, A_END = 9216;
// then (unsigned) [T_MAXWG] arrival words, [T_MAXWG] not-below-threshold counts, [8] status
constexpr int U_FLAG = 0, U_CNT = T_MAXWG, U_STATUS = 2 * T_MAXWG, U_END = 2 * T_MAXWG + 8;
// the prefix of every decoder workspace, [A_END floats | U_END words]: the status words stay where wrnn_taco_status reads them; a kernel's
// tagged vectors follow
constexpr size_t TACO_PREFIX_BYTES = (size_t)A_END * 4 + (size_t)U_END * 4;
static_assert(TACO_PREFIX_BYTES % 8 == 0, "tagged entries are 8-byte aligned");

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

constexpr int R_NWG = 128, R_NWV = R_NWG * NW;
constexpr int R_MAXR = 8;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ float dpp_get(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_get(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
// sum over the 64 lanes, in every lane: quad xor 1, xor 2, half-row mirror, row mirror (16-lane row totals), then the four rows
__device__ __forceinline__ float wave_total(float v)
{
    v += dpp_get<0xB1>(v);
    v += dpp_get<0x4E>(v);
    v += dpp_get<0x141>(v);
    v += dpp_get<0x140>(v);
    return (lane_get(v, 0) + lane_get(v, 16)) + (lane_get(v, 32) + lane_get(v, 48));
}
__device__ __forceinline__ float4 ldw4(const float *w, bool on) { return on ? *reinterpret_cast<const float4 *>(w) : make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float fma4(const float4 a, const float *x, float s)
{
    const float4 b = *reinterpret_cast<const float4 *>(x);
    s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    return s;
}

}  // namespace wrnn
