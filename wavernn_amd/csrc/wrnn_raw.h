// wrnn_raw.h -- the 9-bit RAW sampler of one segment per wave (fatchord_version.py:231-237: softmax -> Categorical, which renormalises ->
// argmax(p / q) over the step's exponential noise), as a device function.  The operation order is the reference's, element by element, and the
// wave reductions are wrnn_device.h's DPP / permlane butterflies (== the __shfl_xor forms bit for bit): the same arithmetic as the RAW samplers
// of wrnn_chain.hip / wrnn_duo.hip, which keep their own copies (their code objects stay as they were measured).  Used by wrnn_sparse.hip.
#pragma once
#include "wrnn_device.h"

namespace wrnn {

// lg[e], qn[e]: logit and noise of class lane + 64 e (512 classes over the 64 lanes); returns the class (every lane the same)
__device__ __forceinline__ int raw_sample512(float (&lg)[8], const float (&qn)[8], int lane)
{
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, lg[e]);
    mx = wave_max64(mx);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { lg[e] = expf(lg[e] - mx); sum += lg[e]; }
    sum = wave_sum64(sum);
    float sum2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { lg[e] = lg[e] / sum; sum2 += lg[e]; }
    sum2 = wave_sum64(sum2);
    float best = -INFINITY;
    int bidx = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float rr = (lg[e] / sum2) / qn[e];
        if (rr > best) { best = rr; bidx = lane + 64 * e; }
    }
    wave_argmax64(best, bidx);
    return bidx;
}

}  // namespace wrnn
