// wrnn_nll.hip -- the loss of a teacher-forced loop call (wrnn_nll, wrnn_nll_host): -log p of every step from the fc3 outputs the call left in
// wrnn_options.logits ([T][n][C]) and the waveform it was fed through wrnn_options.force_x ([n][T]).  float32 arithmetic like the reference's:
// MOL = discretized_mix_logistic_loss (utils/distribution.py:16-84, num_classes 65536, log_scale_min log(1e-14)), RAW = F.cross_entropy
// (train_wavernn.py:83).  ONE workgroup per segment walks that segment's T rows, so a segment's values and its sum are formed by the same
// instructions in the same order whatever rides along; the per-step float32 values are summed in float64, slot by slot and then over the slots
// (below) -- no atomics, two runs give the same bits.  The value formulas are __host__ __device__: wrnn_nll_host runs them on the calling thread.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "wrnn_device.h"

namespace wrnn {

constexpr int NLL_THREADS = 1024;
constexpr int NLL_MIX = 10;            // mixtures of the MoL head (n_classes = 30: logits | means | log-scales)
// Steps in flight per workgroup pass: MOL one 16-lane DPP row per step (lane j < 10 = mixture j: the row's three loads are each 40 contiguous
// bytes), RAW one wave per step (lane k, k + 64, ...: contiguous along the classes).  Slot s owns the steps t = s (mod slots) and adds their values
// in step order into one float64; the segment's sum is the slots' sums added in slot order.  nll_host keeps the same order.
constexpr int NLL_MOL_SLOTS = NLL_THREADS / 16, NLL_RAW_SLOTS = NLL_THREADS / 64;
constexpr int NLL_RAW_VEC = 8;         // float4 per lane that hold a row of <= 2048 classes

struct NllArgs {
    const float *logits, *target;
    const int *seg_len;
    float *nll;
    double *sum;
    int n, T, C;
};

__host__ __device__ inline float nll_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }      // F.softplus (beta 1, threshold 20)
__host__ __device__ inline float nll_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// distribution.py:31-77 for one mixture: the log probability of y under a logistic (mean, log_scale) discretised to 16 bits
__host__ __device__ inline float nll_mol_term(float y, float mean, float log_scale)
{
    const float bin = (float)(1.0 / 65535.0);                  // 1. / (num_classes - 1)
    const float ls = fmaxf(log_scale, -32.23619130191664f);    // log_scale_min = log(1e-14)
    const float cy = y - mean;
    const float inv_stdv = expf(-ls);
    const float plus_in = inv_stdv * (cy + bin), min_in = inv_stdv * (cy - bin), mid_in = inv_stdv * cy;
    const float cdf_delta = nll_sigmoid(plus_in) - nll_sigmoid(min_in);
    const float log_cdf_plus = plus_in - nll_softplus(plus_in);
    const float log_one_minus_cdf_min = -nll_softplus(min_in);
    const float log_pdf_mid = mid_in - ls - 2.f * nll_softplus(mid_in);
    const float inner = cdf_delta > 1e-5f ? logf(fmaxf(cdf_delta, 1e-12f)) : log_pdf_mid - 10.397177190355384f;   // log((num_classes - 1) / 2)
    return y < -0.999f ? log_cdf_plus : (y > 0.999f ? log_one_minus_cdf_min : inner);
}

// the class of a RAW target 2 idx / (C - 1) - 1, clamped into [0, C) whatever the value is (the index addresses the row)
__host__ __device__ inline int nll_raw_class(float x, int C)
{
    const float f = rintf((x + 1.f) * (float)(C - 1) * 0.5f);
    return f >= 0.f ? (f <= (float)(C - 1) ? (int)f : C - 1) : 0;
}

__device__ __forceinline__ float row16_max(float v)
{
    v = wave_max_level<8>(v); v = wave_max_level<4>(v); v = wave_max_level<2>(v); return wave_max_level<1>(v);
}
__device__ __forceinline__ float row16_sum(float v)
{
    v = wave_sum_level<8>(v); v = wave_sum_level<4>(v); v = wave_sum_level<2>(v); return wave_sum_level<1>(v);
}

__device__ __forceinline__ int nll_len(const NllArgs &a, int b)
{
    const int len = a.seg_len ? a.seg_len[b] : a.T;
    return len < 0 ? 0 : (len > a.T ? a.T : len);
}

// the tail of both kernels: zeros past the segment's length, then the slots' sums in slot order
template <int SLOTS>
__device__ __forceinline__ void nll_finish(const NllArgs &a, int b, int len, int slot, bool first, double acc, double *part)
{
    if (a.nll)
        for (int t = len + (int)threadIdx.x; t < a.T; t += NLL_THREADS) a.nll[(size_t)b * a.T + t] = 0.f;
    if (first) part[slot] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < SLOTS; ++i) s += part[i];
        a.sum[b] = s;
    }
}

__global__ __launch_bounds__(NLL_THREADS) void wrnn_nll_mol_kernel(NllArgs a)
{
    __shared__ double part[NLL_MOL_SLOTS];
    const int b = blockIdx.x, slot = threadIdx.x >> 4, j = threadIdx.x & 15;
    const bool act = j < NLL_MIX;
    const int jj = act ? j : 0;
    const int len = nll_len(a, b);
    const size_t stride = (size_t)a.n * 3 * NLL_MIX;
    const float *const rows = a.logits + (size_t)b * 3 * NLL_MIX, *const tg = a.target + (size_t)b * a.T;
    double acc = 0.0;
    // every lane runs every pass (the DPP rows stay whole): a slot past the end re-reads the last counted row and drops the value
    for (int t0 = 0; t0 < len; t0 += NLL_MOL_SLOTS) {
        const int t = t0 + slot, tc = t < len ? t : len - 1;
        const float *const p = rows + (size_t)tc * stride;
        const float lg = p[jj], mean = p[NLL_MIX + jj], ls = p[2 * NLL_MIX + jj], y = tg[tc];
        const float lgm = act ? lg : -INFINITY;
        const float mx = row16_max(lgm);
        const float se = row16_sum(expf(lgm - mx));                          // log_softmax of the mixture logits (:79)
        const float lp = act ? nll_mol_term(y, mean, ls) + (lg - mx - logf(se)) : -INFINITY;
        const float m2 = row16_max(lp);
        const float s2 = row16_sum(expf(lp - m2));                           // log_sum_exp (:6-12)
        const float v = -(m2 + logf(s2));
        if (j == 0 && t < len) {
            if (a.nll) a.nll[(size_t)b * a.T + t] = v;
            acc += (double)v;
        }
    }
    nll_finish<NLL_MOL_SLOTS>(a, b, len, slot, j == 0, acc, part);
}

// VEC: n_classes a multiple of 4 and `logits` 16-byte aligned -- the row is read once, as float4, and stays in registers
template <bool VEC>
__global__ __launch_bounds__(NLL_THREADS) void wrnn_nll_raw_kernel(NllArgs a)
{
    __shared__ double part[NLL_RAW_SLOTS];
    const int b = blockIdx.x, slot = threadIdx.x >> 6, lane = threadIdx.x & 63, C = a.C;
    const int len = nll_len(a, b);
    const float *const tg = a.target + (size_t)b * a.T;
    double acc = 0.0;
    for (int t0 = 0; t0 < len; t0 += NLL_RAW_SLOTS) {
        const int t = t0 + slot, tc = t < len ? t : len - 1;
        const float *const p = a.logits + ((size_t)tc * a.n + b) * C;
        const float hit = p[nll_raw_class(tg[tc], C)];
        float m = -INFINITY, s = 0.f;
        if (VEC) {
            f32x4 r[NLL_RAW_VEC];
#pragma unroll
            for (int i = 0; i < NLL_RAW_VEC; ++i) {
                const int k = 4 * (lane + 64 * i);
                if (k < C) r[i] = *reinterpret_cast<const f32x4 *>(p + k);
                else r[i].x = r[i].y = r[i].z = r[i].w = -INFINITY;
                m = fmaxf(m, fmaxf(fmaxf(r[i].x, r[i].y), fmaxf(r[i].z, r[i].w)));
            }
            m = wave_max64(m);
#pragma unroll
            for (int i = 0; i < NLL_RAW_VEC; ++i) s += (expf(r[i].x - m) + expf(r[i].y - m)) + (expf(r[i].z - m) + expf(r[i].w - m));
        } else {
            for (int k = lane; k < C; k += 64) m = fmaxf(m, p[k]);
            m = wave_max64(m);
            for (int k = lane; k < C; k += 64) s += expf(p[k] - m);            // (the second pass comes out of the cache)
        }
        s = wave_sum64(s);
        const float v = -((hit - m) - logf(s));                               // -log_softmax(logits)[idx]
        if (lane == 0 && t < len) {
            if (a.nll) a.nll[(size_t)b * a.T + t] = v;
            acc += (double)v;
        }
    }
    nll_finish<NLL_RAW_SLOTS>(a, b, len, slot, lane == 0, acc, part);
}

// The caller has checked the arguments (MOL: C == 30; RAW: 2 <= C <= 2048 = 4 * 64 * NLL_RAW_VEC).
hipError_t launch_nll(bool mol, const NllArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.n), block(NLL_THREADS);
    if (mol) hipLaunchKernelGGL(wrnn_nll_mol_kernel, grid, block, 0, stream, a);
    else if ((a.C & 3) == 0 && ((uintptr_t)a.logits & 15) == 0) hipLaunchKernelGGL(wrnn_nll_raw_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(wrnn_nll_raw_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

// the same values by the calling thread (no HIP call); host pointers
void nll_host(bool mol, const NllArgs &a)
{
    const int slots = mol ? NLL_MOL_SLOTS : NLL_RAW_SLOTS, C = a.C;
    for (int b = 0; b < a.n; ++b) {
        int len = a.seg_len ? a.seg_len[b] : a.T;
        len = len < 0 ? 0 : (len > a.T ? a.T : len);
        double part[NLL_MOL_SLOTS > NLL_RAW_SLOTS ? NLL_MOL_SLOTS : NLL_RAW_SLOTS] = {0.0};
        for (int t = 0; t < a.T; ++t) {
            float v = 0.f;
            if (t < len) {
                const float *const p = a.logits + ((size_t)t * a.n + b) * C;
                const float y = a.target[(size_t)b * a.T + t];
                if (mol) {
                    float mx = -INFINITY, se = 0.f, lp[NLL_MIX], m2 = -INFINITY, s2 = 0.f;
                    for (int j = 0; j < NLL_MIX; ++j) mx = fmaxf(mx, p[j]);
                    for (int j = 0; j < NLL_MIX; ++j) se += expf(p[j] - mx);
                    const float lse = logf(se);
                    for (int j = 0; j < NLL_MIX; ++j) {
                        lp[j] = nll_mol_term(y, p[NLL_MIX + j], p[2 * NLL_MIX + j]) + (p[j] - mx - lse);
                        m2 = fmaxf(m2, lp[j]);
                    }
                    for (int j = 0; j < NLL_MIX; ++j) s2 += expf(lp[j] - m2);
                    v = -(m2 + logf(s2));
                } else {
                    float m = -INFINITY, s = 0.f;
                    for (int k = 0; k < C; ++k) m = fmaxf(m, p[k]);
                    for (int k = 0; k < C; ++k) s += expf(p[k] - m);
                    v = -((p[nll_raw_class(y, C)] - m) - logf(s));
                }
                part[t % slots] += (double)v;
            }
            if (a.nll) a.nll[(size_t)b * a.T + t] = v;
        }
        double s = 0.0;
        for (int i = 0; i < slots; ++i) s += part[i];
        a.sum[b] = s;
    }
}

}  // namespace wrnn
