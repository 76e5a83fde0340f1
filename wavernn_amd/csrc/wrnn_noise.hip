// wrnn_noise.hip -- the library's own sampling noise (wrnn_options.noise_lib, wrnn_noise_fill, wrnn_noise_fill_host): Philox4x32-10 keyed by the
// call's seed, one block per (step, four indices, segment id); the value formulas are in wrnn_philox.h.  Output in the layout wrnn_generate*
// documents for `noise`: MOL [steps][11 B] (per step 10 B mixture uniforms, segment-major, then B logistic uniforms), RAW [steps][B][C].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wrnn_device.h"
#include "wrnn_philox.h"

namespace wrnn {

constexpr int NOISE_IDS = 256;      // segment ids handed over by value with one launch (kernel arguments are copied when the launch is enqueued:
struct NoiseIds { uint64_t v[NOISE_IDS]; };   // no device table, nothing asynchronous reads the caller's host array)

// One row = (step, segment); 2^tpr_log2 threads share a row (index quads q, q + 2^tpr_log2, ...), 256 >> tpr_log2 rows per workgroup pass.  A plain
// grid-stride kernel over the rows: no workgroup reads what another wrote.  Segments [b0, b0 + nb) of the B, steps [t0, t0 + nt); row 0 of `out` is step t0.
template <bool MOL>
__global__ __launch_bounds__(256) void wrnn_noise_fill_kernel(float *__restrict__ out, NoiseIds ids, int use_ids, int b0, int nb, int B, int J, int t0, int nt,
                                                              uint64_t seed, int tpr_log2)
{
    const unsigned rows = (unsigned)nt * (unsigned)nb, rpb = 256u >> tpr_log2, tpr = 1u << tpr_log2;
    const unsigned lq = threadIdx.x & (tpr - 1u);
    const unsigned Q = ((unsigned)J + 3u) >> 2;
    for (unsigned row = blockIdx.x * rpb + (threadIdx.x >> tpr_log2); row < rows; row += gridDim.x * rpb) {
        const unsigned tr = row / (unsigned)nb, bl = row - tr * (unsigned)nb, b = (unsigned)b0 + bl;
        const uint64_t id = use_ids ? ids.v[bl] : (uint64_t)b;
        for (unsigned q = lq; q < Q; q += tpr) {
            const PhiloxBlock blk = noise_block(seed, id, t0 + (int)tr, q);
            if (MOL) {
                float *const rowp = out + (size_t)tr * 11u * (unsigned)B;
#pragma unroll
                for (unsigned e = 0; e < 4; ++e) {
                    const unsigned j = 4u * q + e;
                    if (j < 10u) rowp[(size_t)b * 10u + j] = noise_mol_value(blk.w[e]);
                    else if (j == 10u) rowp[(size_t)10u * (unsigned)B + b] = noise_mol_value(blk.w[e]);
                }
            } else {
                float *const p = out + ((size_t)tr * (unsigned)B + b) * (unsigned)J + 4u * q;
                if ((J & 3) == 0) {      // four consecutive outputs, 16-byte aligned with `out`
                    f32x4 v;
                    v.x = noise_raw_value(blk.w[0]); v.y = noise_raw_value(blk.w[1]); v.z = noise_raw_value(blk.w[2]); v.w = noise_raw_value(blk.w[3]);
                    *reinterpret_cast<f32x4 *>(p) = v;
                } else {
#pragma unroll
                    for (unsigned e = 0; e < 4; ++e)
                        if (4u * q + e < (unsigned)J) p[e] = noise_raw_value(blk.w[e]);
                }
            }
        }
    }
}

// steps [t0, t1) of B segments -> out; seg_id: HOST [B] or null (segment b has id b).  Grid sized from the device's CUs.  The caller has checked the arguments.
hipError_t launch_noise_fill(bool mol, int B, int C, int t0, int t1, uint64_t seed, const uint64_t *seg_id, float *out, int n_cus, hipStream_t stream)
{
    const int J = mol ? 11 : C, Q = (J + 3) / 4, nt = t1 - t0;
    int tpr_log2 = 0;
    while ((1 << tpr_log2) < Q && tpr_log2 < 8) ++tpr_log2;
    const long rpb = 256 >> tpr_log2;
    NoiseIds ids;
    for (int i = 0; i < NOISE_IDS; ++i) ids.v[i] = 0;
    const int chunk = seg_id ? NOISE_IDS : B;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        if (seg_id)
            for (int i = 0; i < nb; ++i) ids.v[i] = seg_id[b0 + i];
        long blocks = ((long)nt * nb + rpb - 1) / rpb;
        if (blocks > (long)n_cus * 8) blocks = (long)n_cus * 8;
        if (blocks < 1) blocks = 1;
        if (mol) hipLaunchKernelGGL(wrnn_noise_fill_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, out, ids, seg_id ? 1 : 0, b0, nb, B, J, t0, nt, seed, tpr_log2);
        else hipLaunchKernelGGL(wrnn_noise_fill_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, out, ids, seg_id ? 1 : 0, b0, nb, B, J, t0, nt, seed, tpr_log2);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the same values by the calling thread (no HIP call)
void noise_fill_host(bool mol, int B, int C, int t0, int t1, uint64_t seed, const uint64_t *seg_id, float *out)
{
    const int J = mol ? 11 : C, Q = (J + 3) / 4;
    for (int t = t0; t < t1; ++t)
        for (int b = 0; b < B; ++b) {
            const uint64_t id = seg_id ? seg_id[b] : (uint64_t)b;
            for (int q = 0; q < Q; ++q) {
                const PhiloxBlock blk = noise_block(seed, id, t, (uint32_t)q);
                for (int e = 0; e < 4 && 4 * q + e < J; ++e) {
                    const int j = 4 * q + e;
                    if (mol) out[(size_t)(t - t0) * 11 * B + (j < 10 ? (size_t)b * 10 + j : (size_t)10 * B + b)] = noise_mol_value(blk.w[e]);
                    else out[((size_t)(t - t0) * B + b) * J + j] = noise_raw_value(blk.w[e]);
                }
            }
        }
}

}  // namespace wrnn
