// wrnn_tile_body.inc -- the body of a loop kernel of the 16-segment tile dataflow (wrnn_tile.hip describes it): the LDS carve, then per step the conditioning,
// the I layer, rnn1, rnn2, fc1, fc2, fc3 and the sampling.  Included INSIDE a kernel `template <int MODE> ... (const GenArgs a ...)` of TNT threads, after the
// kernel has defined the matrix products as macros over the names of this body (a, H, F, A, C, K0, w, lane):
//   TILE_STAGE_I(x, dst)                                        W_I . x + b -> dst
//   TILE_STAGE_RNN1(x, hs, dst)  TILE_STAGE_RNN2(x, hs, dst)    one GRU stage on input vector x and state hs, the new h -> dst
//   TILE_STAGE_FC1(x, dst)       TILE_STAGE_FC2(x, dst)         relu(W . x + b) -> dst
//   TILE_FC3_TILE(row0, x, acc)                                 MOL: fc3 rows row0 .. row0 + 15 (consecutive) . x -> f32x4 acc[1]
//   TILE_FC3_GROUP(row0, x, acc)                                RAW: fc3 rows row0 .. row0 + 63 as four interleaved tiles . x -> f32x4 acc[4]
// Text, not a function: wrnn_tile_kernel, which was written first, compiles to the code object it had before wrnn_tile_sparse_kernel shared this body.

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
        TILE_STAGE_I(in0, vb);
        __syncthreads();
        // ---- rnn1 (:210) on xi; the new h1 -> va[0..H), then h1 <- it and x1 = xi + h1 (:212) -> va[0..H)
        TILE_STAGE_RNN1(vb, h1s, va);
        __syncthreads();                                // every wave has read the old h1
        for (int i = tid; i < H * SEG; i += TNT) { const float hn = va[i]; h1s[i] = hn; va[i] = vb[i] + hn; }
        __syncthreads();
        // ---- rnn2 (:213-214) on [x1 | a2]; the new h2 -> vb[0..H) (xi is dead), then h2 <- it and x2 = x1 + h2 (:216) -> vb[0..H)
        TILE_STAGE_RNN2(va, h2s, vb);
        __syncthreads();
        for (int i = tid; i < H * SEG; i += TNT) { const float hn = vb[i]; h2s[i] = hn; vb[i] = va[i] + hn; }
        __syncthreads();
        // ---- fc1 (:217-218) on [x2 | a3] -> va[0..F), a4 behind it (va is free: x1 | a2 were last read above)
        TILE_STAGE_FC1(vb, va);
        for (int s = w; s < nb; s += TNW) {             // a4
            const int p = a.seg_pos[b0 + s] + t;
            const bool live = p < a.seg_lim[b0 + s];
            const float *arow = a.aux + (size_t)((live ? p : 0) / a.hop) * 4 * A;
            for (int k = lane; k < A; k += 64) va[(F + k) * SEG + s] = live ? arow[3 * A + k] : 0.f;
        }
        __syncthreads();
        // ---- fc2 (:220-221) on [y1 | a4] -> vb[0..F)
        TILE_STAGE_FC2(va, vb);
        __syncthreads();
        // ---- fc3 (:223) and the sampling, per segment
        if (MODE == 1) {                                // utils/distribution.py:102-121 (C = 30: 10 mixtures); logits -> red[c][seg]
            for (int tile = w; tile * 16 < C; tile += TNW) {
                f32x4 acc[1];
                TILE_FC3_TILE(tile * 16, vb, acc);
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
                    TILE_FC3_GROUP(grp * 64, vb, acc);
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
        if (a.progress) {                               // (uniform) a watched call: this tile's word, once per progress_every steps and at the end
            const int done = t + 1;
            if (done % a.progress_every == 0 || done == T) publish_progress(a.progress + blockIdx.x, (unsigned)done, tid);
        }
    }
