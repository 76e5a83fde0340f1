// wrnn_cbhg.hip -- Tacotron's encoder and post-net on MI355X (gfx950) around the two persistent kernels of wrnn_taco.hip: the embedding
// and the encoder pre-net (reference models/tacotron.py:24-39, :141-155), both CBHGs in front of their GRU (:57-139: conv bank of
// BatchNormConv :43-54, max-pool, two projections, residual, pre_highway, highways, the two W_ih products), `encoder_proj` and
// `post_proj` (:403-404, :424-425).  Once per sentence (wrnn_taco_encode / wrnn_taco_postnet), or once for a LIST of sentences
// (wrnn_taco_encode_many / wrnn_taco_postnet_many: K-cbhg-many below); ordinary data-parallel kernels, no cooperative launch, no
// inter-workgroup wait.
// All arithmetic is float32 on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation); activations travel as
// [position][channel] rows.
//
// K-cbhg-1  wrnn_cbhg_conv_kernel / wrnn_cbhg_bank_kernel: a conv1d of width k (padding k / 2, zero padded, no bias) as an im2col GEMM.
//           The weight is repacked tap-major on the host, W'[co][j * Cin + ci], so that the im2col row of position p is rows
//           p - k/2 .. p - k/2 + k - 1 of the input, one after another: out[p][co] = sum_j sum_ci W[co][ci][j] x[p + j - k/2][ci] for
//           both parities of k (for even k conv1d returns n + 1 positions and the reference keeps the first n).  A workgroup owns
//           16 positions x 16 output channels; the window of 16 + k - 1 input rows is staged in LDS in slices of <= 256 channels and
//           the four waves split every slice's (tap, 16-channel chunk) items, two accumulators per wave, so the longest single
//           chain of the K = 6144 projection is 192 steps; the eight partial tiles are summed in a fixed order.  Epilogue:
//           [bias] -> [ReLU] -> [eval-mode BatchNorm as a per-channel scale / shift: it FOLLOWS the ReLU, :50-53, so it cannot be
//           folded into the weights] -> [+ residual].  The loader can form max_pool1d(2, 1, 1)[:n] on the fly
//           (out[p] = max(in[p-1], in[p]); the pool pads with -inf, so out[0] = in[0]; the conv that follows pads THAT with 0),
//           read a [channel][position] tensor (the decoder's mel), or gather rows by index (the embedding).  The bank kernel is the
//           same body on a grid of (position tile, channel tile, bank index).
// K-cbhg-2  wrnn_rowlin_kernel: [n][K] -> [n][M], the same body with one tap: optional bias, ReLU, gathered input rows.  Pre-net,
//           pre_highway, gi = W_ih x + b_ih of both directions, encoder_proj, post_proj.
// K-cbhg-3  wrnn_highway_kernel: all highways (:7-21: x <- sigmoid(W2 x + b2) relu(W1 x + b1) + (1 - sigmoid(..)) x) of a 16-position
//           tile in LDS, wave w owns channels [32w, 32w + 32) with the full K = 128 (no cross-wave sum); library expf, exact division.
// K-cbhg-many  wrnn_cbhg_bank_many_kernel / wrnn_cbhg_conv_many_kernel / wrnn_rowlin_many_kernel / wrnn_highway_many_kernel: the same tile
//           bodies for up to 64 sentences in one launch.  The sentences' rows lie one after another in every [position][channel] tensor;
//           a sentence table (lengths, first rows, first tiles, the post-net's per-sentence input pointers) is a kernel argument;
//           blockIdx.x runs over the concatenated tile list, the workgroup finds (sentence, tile in sentence), rebases a private copy of
//           the arguments to the sentence and calls the body with the sentence-relative position -- tiles restart at position 0 of every
//           sentence, so windows, the pool's and the conv's padding and the residual never see a neighbour's rows and every output
//           element has the operands and the summation order of the single-sentence launch: bitwise the same result.
// The GRU itself is wrnn_bigru / wrnn_bigru_many (wrnn_taco.hip), called from here.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "wrnn_device.h"
#include "../../include/wavernn_amd.h"

namespace wrnn {

constexpr int CB_C = 128;                       // CBHG `channels`: conv bank outputs, highway and GRU width (wrnn_bigru's hidden size)
constexpr int CB_NP = 16;                       // positions per workgroup (MFMA N)
constexpr int CB_MAXK = 16;                     // widest conv of a bank
constexpr int CB_CC = 256;                      // input channels per LDS stage
constexpr int CB_LD = CB_CC + 4;                // LDS row stride of the staged window
constexpr int CB_ROWS = CB_NP + CB_MAXK - 1;    // rows of the widest window
constexpr int CB_LDX = CB_C + 4;                // LDS row stride of the highway tiles
constexpr int CB_MAXHW = 4;
constexpr int CB_HW_STRIDE = 2 * CB_C * CB_C + 2 * CB_C;   // one highway layer: W1, W2, b1, b2
enum { CB_RELU = 1, CB_POOL = 2, CB_IN_CMAJOR = 4, CB_RES_CMAJOR = 8 };

struct ConvArgs {
    const float *in;            // [n][ldin] rows ([rows_in_table][ldin] with `ids`), or [Cin][n] with CB_IN_CMAJOR
    const int *ids;             // optional [n]: input row of position p (taps == 1); an index outside the table reads zeros
    const float *w;             // [Cout][taps * Cin], tap-major
    const float *bias;          // optional [Cout]
    const float *scale, *shift; // optional [Cout] (BatchNorm after the ReLU)
    const float *res;           // optional residual [n][ldres], or [Cout][n] with CB_RES_CMAJOR
    float *out;                 // [n][ldo]
    int n, Cin, Cout, taps, ldin, ldres, ldo, table_rows, flags;
};

__device__ __forceinline__ float4 cb_load_in(const ConvArgs &a, int p, int c)
{
    if (a.flags & CB_IN_CMAJOR) {
        const float *q = a.in + (size_t)c * a.n + p;
        const size_t n = (size_t)a.n;
        return make_float4(q[0], q[n], q[2 * n], q[3 * n]);
    }
    size_t row = (size_t)p;
    if (a.ids) {
        const int id = a.ids[p];
        if (id < 0 || id >= a.table_rows) return make_float4(0.f, 0.f, 0.f, 0.f);
        row = (size_t)id;
    }
    float4 v = *reinterpret_cast<const float4 *>(a.in + row * a.ldin + c);
    if ((a.flags & CB_POOL) && p > 0) {
        const float4 u = *reinterpret_cast<const float4 *>(a.in + (row - 1) * a.ldin + c);
        v.x = fmaxf(u.x, v.x); v.y = fmaxf(u.y, v.y); v.z = fmaxf(u.z, v.z); v.w = fmaxf(u.w, v.w);
    }
    return v;
}

__device__ __forceinline__ f32x4 cb_mfma4(const float4 av, const float4 bv, f32x4 acc)
{
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
}

// positions [p0, p0 + 16) x output channels [co0, co0 + 16) of one conv / linear layer
__device__ __forceinline__ void cb_conv_tile(const ConvArgs &a, int p0, int co0)
{
    __shared__ __attribute__((aligned(16))) float XS[CB_ROWS * CB_LD];
    __shared__ float PART[NW * 256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, kq = lane >> 4;
    const int k = a.taps, pad = k / 2, rows = CB_NP + k - 1, Cin = a.Cin, n = a.n;
    const float *wrow = a.w + (size_t)(co0 + fi) * k * Cin + 4 * kq;       // lane: A[i = fi][4 kq ..] of every 16-wide chunk
    const float *brow = XS + fi * CB_LD + 4 * kq;                           //       B[4 kq ..][j = fi]
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Cin; c0 += CB_CC) {
        const int cc = Cin - c0 < CB_CC ? Cin - c0 : CB_CC, q4 = cc >> 2;
        for (int q = tid; q < rows * q4; q += NT) {
            const int r = q / q4, c4 = (q - r * q4) * 4;
            const int p = p0 + r - pad;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p >= 0 && p < n) v = cb_load_in(a, p, c0 + c4);
            *reinterpret_cast<float4 *>(XS + r * CB_LD + c4) = v;
        }
        __syncthreads();
        const int nch = cc >> 4, items = k * nch;
        for (int it = w; it < items; it += 2 * NW) {
            {
                const int j = it / nch, ch = it - j * nch;
                const float4 av = *reinterpret_cast<const float4 *>(wrow + (size_t)j * Cin + c0 + ch * 16);
                const float4 bv = *reinterpret_cast<const float4 *>(brow + j * CB_LD + ch * 16);
                acc0 = cb_mfma4(av, bv, acc0);
            }
            const int it2 = it + NW;
            if (it2 < items) {
                const int j = it2 / nch, ch = it2 - j * nch;
                const float4 av = *reinterpret_cast<const float4 *>(wrow + (size_t)j * Cin + c0 + ch * 16);
                const float4 bv = *reinterpret_cast<const float4 *>(brow + j * CB_LD + ch * 16);
                acc1 = cb_mfma4(av, bv, acc1);
            }
        }
        __syncthreads();
    }
    {                                                                       // D reg v: channel (lane >> 4) * 4 + v, position lane & 15
        const f32x4 d = acc0 + acc1;
        float *pp = PART + w * 256 + (kq * 4) * 16 + fi;
        pp[0] = d[0]; pp[16] = d[1]; pp[32] = d[2]; pp[48] = d[3];
    }
    __syncthreads();
    const int cl = tid & 15, pl = tid >> 4, p = p0 + pl, co = co0 + cl;
    if (p >= n) return;
    float v = ((PART[cl * 16 + pl] + PART[256 + cl * 16 + pl]) + PART[512 + cl * 16 + pl]) + PART[768 + cl * 16 + pl];
    if (a.bias) v += a.bias[co];
    if (a.flags & CB_RELU) v = fmaxf(v, 0.f);
    if (a.scale) v = fmaf(v, a.scale[co], a.shift[co]);
    if (a.res) v += (a.flags & CB_RES_CMAJOR) ? a.res[(size_t)co * n + p] : a.res[(size_t)p * a.ldres + co];
    a.out[(size_t)p * a.ldo + co] = v;
}

__global__ __launch_bounds__(NT) void wrnn_cbhg_conv_kernel(const ConvArgs a) { cb_conv_tile(a, blockIdx.x * CB_NP, blockIdx.y * 16); }

__global__ __launch_bounds__(NT) void wrnn_rowlin_kernel(const ConvArgs a) { cb_conv_tile(a, blockIdx.x * CB_NP, blockIdx.y * 16); }

// bank index z = blockIdx.z: width z + 1; the weights of all widths lie one after another (width k at 128 Cin k (k - 1) / 2 floats), the
// scale / shift pairs as [z][2][128], the outputs side by side: channel z * 128 + co of a.out
__global__ __launch_bounds__(NT) void wrnn_cbhg_bank_kernel(const ConvArgs b)
{
    ConvArgs a = b;
    const int z = blockIdx.z;
    a.taps = z + 1;
    a.w = b.w + (size_t)CB_C * b.Cin * (z * (z + 1) / 2);
    a.scale = b.scale + (size_t)z * 2 * CB_C;
    a.shift = a.scale + CB_C;
    a.out = b.out + (size_t)z * CB_C;
    cb_conv_tile(a, blockIdx.x * CB_NP, blockIdx.y * 16);
}

// Several sentences in one launch (wrnn_taco_encode_many / wrnn_taco_postnet_many).  The sentence table travels with the launch as a kernel argument:
// sentence s has n[s] positions, owns rows [row0[s], row0[s] + n[s]) of every concatenated [row][channel] tensor and tiles [tile0[s], tile0[s + 1]) of
// the grid's x; src[s] is its own [n_mels][N_s] tensor (the post-net's input and residual).
constexpr int CB_MANY = WRNN_TACO_FRONT_MANY_MAX;
struct FrontTab {
    int n_sent;
    int n[CB_MANY], row0[CB_MANY], tile0[CB_MANY + 1];
    const float *src[CB_MANY];
};

// the sentence that owns tile `b` of the concatenated tile list (tile0 is increasing: every sentence has at least one tile)
__device__ __forceinline__ int cb_sentence_of(const FrontTab &t, int b)
{
    int lo = 0, hi = t.n_sent;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.tile0[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// the arguments of the single-sentence launch on sentence s: tiles, windows, the pool's and the conv's padding and the residual are then relative to
// the sentence, and no load or store leaves its rows
__device__ __forceinline__ ConvArgs cb_rebase(const ConvArgs &b, const FrontTab &t, int s)
{
    ConvArgs a = b;
    const size_t r0 = (size_t)t.row0[s];
    a.n = t.n[s];
    if (b.flags & CB_IN_CMAJOR) a.in = t.src[s];
    else if (b.ids) a.ids = b.ids + r0;                                     // (`in` is the table the ids index)
    else a.in = b.in + r0 * b.ldin;
    if (b.res) a.res = (b.flags & CB_RES_CMAJOR) ? t.src[s] : b.res + r0 * b.ldres;
    a.out = b.out + r0 * b.ldo;
    return a;
}

__global__ __launch_bounds__(NT) void wrnn_cbhg_conv_many_kernel(const ConvArgs b, const FrontTab t)
{
    const int s = cb_sentence_of(t, blockIdx.x);
    const ConvArgs a = cb_rebase(b, t, s);
    cb_conv_tile(a, (blockIdx.x - t.tile0[s]) * CB_NP, blockIdx.y * 16);
}

__global__ __launch_bounds__(NT) void wrnn_rowlin_many_kernel(const ConvArgs b, const FrontTab t)
{
    const int s = cb_sentence_of(t, blockIdx.x);
    const ConvArgs a = cb_rebase(b, t, s);
    cb_conv_tile(a, (blockIdx.x - t.tile0[s]) * CB_NP, blockIdx.y * 16);
}

__global__ __launch_bounds__(NT) void wrnn_cbhg_bank_many_kernel(const ConvArgs b, const FrontTab t)
{
    const int s = cb_sentence_of(t, blockIdx.x);
    ConvArgs a = cb_rebase(b, t, s);
    const int z = blockIdx.z;                                               // as wrnn_cbhg_bank_kernel
    a.taps = z + 1;
    a.w = b.w + (size_t)CB_C * b.Cin * (z * (z + 1) / 2);
    a.scale = b.scale + (size_t)z * 2 * CB_C;
    a.shift = a.scale + CB_C;
    a.out += (size_t)z * CB_C;
    cb_conv_tile(a, (blockIdx.x - t.tile0[s]) * CB_NP, blockIdx.y * 16);
}

struct HighwayArgs {
    const float *in;            // [n][128]
    float *out;                 // [n][128] (may be `in`: a workgroup reads and writes its own rows only)
    const float *hw;            // [layers][W1 128x128 | W2 128x128 | b1 128 | b2 128]
    int n, layers;
};

__device__ __forceinline__ f32x4 cb_tile128(const float *W, int row0, const float *act, int lane)
{
    float af[AF];
    load_afrag(af, W, CB_C, row0 + (lane & 15), true, 4 * (lane >> 4));
    return mfma_tile(af, act + (lane & 15) * CB_LDX + 4 * (lane >> 4));
}

// positions [p0, p0 + 16) through all highways
__device__ __forceinline__ void cb_highway_tile(const HighwayArgs &a, int p0)
{
    __shared__ __attribute__((aligned(16))) float XA[CB_NP * CB_LDX];
    __shared__ __attribute__((aligned(16))) float XB[CB_NP * CB_LDX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.n;
    for (int q = tid; q < CB_NP * (CB_C / 4); q += NT) {
        const int r = q / (CB_C / 4), c4 = (q % (CB_C / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p0 + r < n) v = *reinterpret_cast<const float4 *>(a.in + (size_t)(p0 + r) * CB_C + c4);
        *reinterpret_cast<float4 *>(XA + r * CB_LDX + c4) = v;
    }
    __syncthreads();
    float *cur = XA, *nxt = XB;
    const int fi = lane & 15, rq = (lane >> 4) * 4;
    for (int l = 0; l < a.layers; ++l) {
        const float *W1 = a.hw + (size_t)l * CB_HW_STRIDE, *W2 = W1 + CB_C * CB_C, *b1 = W2 + CB_C * CB_C, *b2 = b1 + CB_C;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int row0 = 32 * w + 16 * tt;
            const f32x4 d1 = cb_tile128(W1, row0, cur, lane);
            const f32x4 d2 = cb_tile128(W2, row0, cur, lane);
            const float4 c1 = *reinterpret_cast<const float4 *>(b1 + row0 + rq);
            const float4 c2 = *reinterpret_cast<const float4 *>(b2 + row0 + rq);
            const float4 x = *reinterpret_cast<const float4 *>(cur + fi * CB_LDX + row0 + rq);
            const float g0 = 1.0f / (1.0f + expf(-(d2[0] + c2.x))), g1 = 1.0f / (1.0f + expf(-(d2[1] + c2.y)));
            const float g2 = 1.0f / (1.0f + expf(-(d2[2] + c2.z))), g3 = 1.0f / (1.0f + expf(-(d2[3] + c2.w)));
            float4 y;
            y.x = g0 * fmaxf(d1[0] + c1.x, 0.f) + (1.0f - g0) * x.x;
            y.y = g1 * fmaxf(d1[1] + c1.y, 0.f) + (1.0f - g1) * x.y;
            y.z = g2 * fmaxf(d1[2] + c1.z, 0.f) + (1.0f - g2) * x.z;
            y.w = g3 * fmaxf(d1[3] + c1.w, 0.f) + (1.0f - g3) * x.w;
            *reinterpret_cast<float4 *>(nxt + fi * CB_LDX + row0 + rq) = y;
        }
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
    }
    for (int q = tid; q < CB_NP * (CB_C / 4); q += NT) {
        const int r = q / (CB_C / 4), c4 = (q % (CB_C / 4)) * 4;
        if (p0 + r < n) *reinterpret_cast<float4 *>(a.out + (size_t)(p0 + r) * CB_C + c4) = *reinterpret_cast<const float4 *>(cur + r * CB_LDX + c4);
    }
}

__global__ __launch_bounds__(NT) void wrnn_highway_kernel(const HighwayArgs a) { cb_highway_tile(a, blockIdx.x * CB_NP); }

__global__ __launch_bounds__(NT) void wrnn_highway_many_kernel(const HighwayArgs b, const FrontTab t)
{
    const int s = cb_sentence_of(t, blockIdx.x);
    HighwayArgs a = b;
    a.in = b.in + (size_t)t.row0[s] * CB_C;
    a.out = b.out + (size_t)t.row0[s] * CB_C;
    a.n = t.n[s];
    cb_highway_tile(a, (blockIdx.x - t.tile0[s]) * CB_NP);
}

}  // namespace wrnn

using namespace wrnn;

// ---------------------------------------------------------------------------------------------------------
// C ABI (declared in include/wavernn_amd.h); messages through wrnn_taco_last_error()
// ---------------------------------------------------------------------------------------------------------
void taco_err(const char *fmt, ...);                                    // wrnn_taco.hip
#define CB_FAIL(code, ...)       \
    do {                         \
        taco_err(__VA_ARGS__);   \
        return code;             \
    } while (0)
#define CB_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) CB_FAIL(WRNN_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct CbhgDev {
    int K, Cin, P1, P2, layers;
    const float *bank_w, *bank_ss, *p1_w, *p1_ss, *p2_w, *p2_ss, *pre_hw_w, *hw;
    const float *w_ih[2], *b_ih[2], *w_hh[2], *b_hh[2];
};

struct wrnn_taco_front {
    int device;
    int n_symbols, E, PN1, D, n_mels, fft;
    float *dev;
    const float *emb, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *enc_proj_w, *post_proj_w;
    CbhgDev enc, post;
    size_t w_t0, w_x, w_bank;                  // workspace row widths (floats): pre-net fc1 / projection 1, CBHG input / projection 2, bank
};

static bool cb_mult16(int v) { return v >= 16 && v <= 4096 && (v & 15) == 0; }

// dims and (with `pointers`) pointers of one CBHG; `what` names it in the message.  Returns 0 or WRNN_ERR_ARG.
static int cb_check(const wrnn_cbhg_weights *c, const char *what, bool pointers)
{
    if (c->K < 1 || c->K > CB_MAXK) CB_FAIL(WRNN_ERR_ARG, "%s: conv bank of %d (1..%d)", what, c->K, CB_MAXK);
    if (c->channels != CB_C) CB_FAIL(WRNN_ERR_ARG, "%s: highway / GRU width %d (this build: %d, the width of wrnn_bigru)", what, c->channels, CB_C);
    if (!cb_mult16(c->in_channels) || !cb_mult16(c->proj1_channels) || !cb_mult16(c->proj2_channels))
        CB_FAIL(WRNN_ERR_ARG, "%s: channel counts must be multiples of 16 in 16..4096 (input %d, projections %d / %d)", what, c->in_channels,
                c->proj1_channels, c->proj2_channels);
    if (c->proj2_channels != c->in_channels)
        CB_FAIL(WRNN_ERR_ARG, "%s: the residual needs conv_project2's %d channels to equal the input's %d", what, c->proj2_channels, c->in_channels);
    if (pointers && (c->proj2_channels != CB_C) != (c->pre_highway_w != nullptr))
        CB_FAIL(WRNN_ERR_ARG, "%s: pre_highway must be given exactly when conv_project2 has other than %d channels (%d)", what, CB_C, c->proj2_channels);
    if (c->num_highways < 0 || c->num_highways > CB_MAXHW) CB_FAIL(WRNN_ERR_ARG, "%s: %d highways (0..%d)", what, c->num_highways, CB_MAXHW);
    if (!pointers) return WRNN_OK;
    bool ok = c->proj1_conv_w && c->proj1_bn_w && c->proj1_bn_b && c->proj1_bn_mean && c->proj1_bn_var && c->proj2_conv_w && c->proj2_bn_w &&
              c->proj2_bn_b && c->proj2_bn_mean && c->proj2_bn_var && c->rnn_w_ih && c->rnn_w_hh && c->rnn_b_ih && c->rnn_b_hh && c->rnn_w_ih_rev &&
              c->rnn_w_hh_rev && c->rnn_b_ih_rev && c->rnn_b_hh_rev;
    for (int i = 0; i < c->K; ++i) ok = ok && c->bank_conv_w[i] && c->bank_bn_w[i] && c->bank_bn_b[i] && c->bank_bn_mean[i] && c->bank_bn_var[i];
    for (int i = 0; i < c->num_highways; ++i) ok = ok && c->highway_w1[i] && c->highway_b1[i] && c->highway_w2[i] && c->highway_b2[i];
    if (!ok) CB_FAIL(WRNN_ERR_ARG, "%s: NULL weight pointer", what);
    return WRNN_OK;
}

static int cb_check_front(const wrnn_taco_front_weights *w, wrnn_taco_front **out, bool pointers)
{
    if (!w || !out) CB_FAIL(WRNN_ERR_ARG, "NULL argument");
    if (w->struct_bytes != sizeof(wrnn_taco_front_weights)) CB_FAIL(WRNN_ERR_ARG, "struct size mismatch (header / library versions differ)");
    if (w->n_symbols < 1 || !cb_mult16(w->embed_dims) || !cb_mult16(w->prenet1) || !cb_mult16(w->prenet2) || !cb_mult16(w->encoder_proj_dims) ||
        !cb_mult16(w->n_mels) || !cb_mult16(w->fft_bins))
        CB_FAIL(WRNN_ERR_ARG, "bad dims: %d symbols; embedding %d, pre-net %d / %d, encoder_proj %d, n_mels %d, fft_bins %d must be multiples of 16 in 16..4096",
                w->n_symbols, w->embed_dims, w->prenet1, w->prenet2, w->encoder_proj_dims, w->n_mels, w->fft_bins);
    if (pointers && (!w->embedding || !w->prenet_fc1_w || !w->prenet_fc1_b || !w->prenet_fc2_w || !w->prenet_fc2_b || !w->encoder_proj_w || !w->post_proj_w))
        CB_FAIL(WRNN_ERR_ARG, "NULL weight pointer");
    int rc = cb_check(&w->encoder_cbhg, "encoder.cbhg", pointers);
    if (rc == WRNN_OK) rc = cb_check(&w->postnet, "postnet", pointers);
    if (rc != WRNN_OK) return rc;
    if (w->encoder_cbhg.in_channels != w->prenet2)
        CB_FAIL(WRNN_ERR_ARG, "encoder.cbhg takes %d channels, the pre-net gives %d", w->encoder_cbhg.in_channels, w->prenet2);
    if (w->postnet.in_channels != w->n_mels) CB_FAIL(WRNN_ERR_ARG, "postnet takes %d channels, n_mels is %d", w->postnet.in_channels, w->n_mels);
    return WRNN_OK;
}

// the dims of `w` and the workspace row widths that follow from them
static void cb_set_dims(wrnn_taco_front *f, const wrnn_taco_front_weights *w, int device)
{
    f->device = device;
    f->n_symbols = w->n_symbols; f->E = w->embed_dims; f->PN1 = w->prenet1; f->D = w->encoder_proj_dims; f->n_mels = w->n_mels; f->fft = w->fft_bins;
    const wrnn_cbhg_weights *c[2] = {&w->encoder_cbhg, &w->postnet};
    CbhgDev *d[2] = {&f->enc, &f->post};
    for (int i = 0; i < 2; ++i) { d[i]->K = c[i]->K; d[i]->Cin = c[i]->in_channels; d[i]->P1 = c[i]->proj1_channels; d[i]->P2 = c[i]->proj2_channels; d[i]->layers = c[i]->num_highways; }
    auto mx = [](size_t a, size_t b) { return a > b ? a : b; };
    f->w_t0 = mx((size_t)f->PN1, mx((size_t)f->enc.P1, (size_t)f->post.P1));
    f->w_x = mx((size_t)f->enc.Cin, (size_t)f->post.Cin);
    f->w_bank = (size_t)CB_C * mx((size_t)f->enc.K, (size_t)f->post.K);
}

// Test hook: a handle that holds the DIMS of `w` and nothing else (device -1, no weights; no weight pointer of `w` is read).  The size queries answer on
// it; every entry point that would launch fails on it with WRNN_ERR_NO_DEVICE -- behind its argument checks, which is what the handle is for.
extern "C" int wrnn_taco_front_debug_host_handle(const wrnn_taco_front_weights *w, wrnn_taco_front **out)
{
    const int rc = cb_check_front(w, out, false);
    if (rc != WRNN_OK) return rc;
    wrnn_taco_front *f = new wrnn_taco_front();
    cb_set_dims(f, w, -1);
    *out = f;
    return WRNN_OK;
}

extern "C" int wrnn_taco_front_create(const wrnn_taco_front_weights *w, int device, wrnn_taco_front **out)
{
    const int rc = cb_check_front(w, out, true);
    if (rc != WRNN_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        CB_FAIL(WRNN_ERR_NO_DEVICE, "no HIP device %d (count %d)", device, ndev);
    DeviceGuard dg(device);
    CB_HIP(dg.err);

    std::vector<float> h, tmp, bn[4];
    hipError_t cperr = hipSuccess;
    auto fetch = [&](std::vector<float> &dst, const float *src, size_t cnt) {                    // device -> host
        dst.resize(cnt);
        const hipError_t e = hipMemcpy(dst.data(), src, cnt * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess && cperr == hipSuccess) cperr = e;
    };
    auto reserve = [&](size_t cnt) { const size_t o = (h.size() + 63) / 64 * 64; h.resize(o + cnt); return o; };
    auto put = [&](const float *src, size_t cnt) { fetch(tmp, src, cnt); const size_t o = reserve(cnt); memcpy(h.data() + o, tmp.data(), cnt * 4); return o; };
    // conv weight (Cout, Cin, k) -> tap-major [Cout][k][Cin] at h[o ..]
    auto put_conv = [&](size_t o, const float *src, int Cout, int Cin, int k) {
        fetch(tmp, src, (size_t)Cout * Cin * k);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Cin; ++ci)
                for (int j = 0; j < k; ++j) h[o + ((size_t)co * k + j) * Cin + ci] = tmp[((size_t)co * Cin + ci) * k + j];
    };
    // eval-mode BatchNorm (eps = 1e-5) as scale / shift in float32: s = w / sqrt(var + eps), t = b - mean * s -> h[o .. o + 2 C)
    auto put_bn = [&](size_t o, const float *bw, const float *bb, const float *bm, const float *bv, int C) {
        fetch(bn[0], bw, C); fetch(bn[1], bb, C); fetch(bn[2], bm, C); fetch(bn[3], bv, C);
        for (int c = 0; c < C; ++c) {
            const float s = bn[0][c] / sqrtf(bn[3][c] + 1e-5f);
            h[o + c] = s;
            h[o + C + c] = bn[1][c] - bn[2][c] * s;
        }
    };
    struct Off { size_t bank_w, bank_ss, p1_w, p1_ss, p2_w, p2_ss, pre_hw, hw, w_ih[2], b_ih[2], w_hh[2], b_hh[2]; };
    auto put_cbhg = [&](const wrnn_cbhg_weights &c) {
        Off o;
        const int K = c.K, Cin = c.in_channels;
        o.bank_w = reserve((size_t)CB_C * Cin * (K * (K + 1) / 2));
        o.bank_ss = reserve((size_t)K * 2 * CB_C);
        for (int z = 0; z < K; ++z) {
            put_conv(o.bank_w + (size_t)CB_C * Cin * (z * (z + 1) / 2), c.bank_conv_w[z], CB_C, Cin, z + 1);
            put_bn(o.bank_ss + (size_t)z * 2 * CB_C, c.bank_bn_w[z], c.bank_bn_b[z], c.bank_bn_mean[z], c.bank_bn_var[z], CB_C);
        }
        o.p1_w = reserve((size_t)c.proj1_channels * K * CB_C * 3);
        put_conv(o.p1_w, c.proj1_conv_w, c.proj1_channels, K * CB_C, 3);
        o.p1_ss = reserve(2 * (size_t)c.proj1_channels);
        put_bn(o.p1_ss, c.proj1_bn_w, c.proj1_bn_b, c.proj1_bn_mean, c.proj1_bn_var, c.proj1_channels);
        o.p2_w = reserve((size_t)c.proj2_channels * c.proj1_channels * 3);
        put_conv(o.p2_w, c.proj2_conv_w, c.proj2_channels, c.proj1_channels, 3);
        o.p2_ss = reserve(2 * (size_t)c.proj2_channels);
        put_bn(o.p2_ss, c.proj2_bn_w, c.proj2_bn_b, c.proj2_bn_mean, c.proj2_bn_var, c.proj2_channels);
        o.pre_hw = c.pre_highway_w ? put(c.pre_highway_w, (size_t)CB_C * c.proj2_channels) : 0;
        o.hw = reserve((size_t)CB_MAXHW * CB_HW_STRIDE);
        for (int l = 0; l < c.num_highways; ++l) {
            const size_t b = o.hw + (size_t)l * CB_HW_STRIDE;
            fetch(tmp, c.highway_w1[l], CB_C * CB_C); memcpy(h.data() + b, tmp.data(), CB_C * CB_C * 4);
            fetch(tmp, c.highway_w2[l], CB_C * CB_C); memcpy(h.data() + b + CB_C * CB_C, tmp.data(), CB_C * CB_C * 4);
            fetch(tmp, c.highway_b1[l], CB_C); memcpy(h.data() + b + 2 * CB_C * CB_C, tmp.data(), CB_C * 4);
            fetch(tmp, c.highway_b2[l], CB_C); memcpy(h.data() + b + 2 * CB_C * CB_C + CB_C, tmp.data(), CB_C * 4);
        }
        o.w_ih[0] = put(c.rnn_w_ih, 3 * CB_C * CB_C); o.w_ih[1] = put(c.rnn_w_ih_rev, 3 * CB_C * CB_C);
        o.b_ih[0] = put(c.rnn_b_ih, 3 * CB_C); o.b_ih[1] = put(c.rnn_b_ih_rev, 3 * CB_C);
        o.w_hh[0] = put(c.rnn_w_hh, 3 * CB_C * CB_C); o.w_hh[1] = put(c.rnn_w_hh_rev, 3 * CB_C * CB_C);
        o.b_hh[0] = put(c.rnn_b_hh, 3 * CB_C); o.b_hh[1] = put(c.rnn_b_hh_rev, 3 * CB_C);
        return o;
    };
    const size_t o_emb = put(w->embedding, (size_t)w->n_symbols * w->embed_dims);
    const size_t o_f1w = put(w->prenet_fc1_w, (size_t)w->prenet1 * w->embed_dims), o_f1b = put(w->prenet_fc1_b, w->prenet1);
    const size_t o_f2w = put(w->prenet_fc2_w, (size_t)w->prenet2 * w->prenet1), o_f2b = put(w->prenet_fc2_b, w->prenet2);
    const size_t o_ep = put(w->encoder_proj_w, (size_t)w->encoder_proj_dims * 2 * CB_C), o_pp = put(w->post_proj_w, (size_t)w->fft_bins * 2 * CB_C);
    const Off oe = put_cbhg(w->encoder_cbhg), op = put_cbhg(w->postnet);
    reserve(64);
    if (cperr != hipSuccess) CB_FAIL(WRNN_ERR_HIP, "reading the weights from the device failed: %s", hipGetErrorString(cperr));

    wrnn_taco_front *f = new wrnn_taco_front();
    hipError_t e = hipMalloc((void **)&f->dev, h.size() * 4);
    if (e != hipSuccess) { delete f; CB_FAIL(WRNN_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e)); }
    e = hipMemcpy(f->dev, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(f->dev); delete f; CB_FAIL(WRNN_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e)); }
    cb_set_dims(f, w, device);
    f->emb = f->dev + o_emb; f->fc1_w = f->dev + o_f1w; f->fc1_b = f->dev + o_f1b; f->fc2_w = f->dev + o_f2w; f->fc2_b = f->dev + o_f2b;
    f->enc_proj_w = f->dev + o_ep; f->post_proj_w = f->dev + o_pp;
    auto fill = [&](CbhgDev &d, const wrnn_cbhg_weights &c, const Off &o) {
        d.bank_w = f->dev + o.bank_w; d.bank_ss = f->dev + o.bank_ss; d.p1_w = f->dev + o.p1_w; d.p1_ss = f->dev + o.p1_ss;
        d.p2_w = f->dev + o.p2_w; d.p2_ss = f->dev + o.p2_ss; d.pre_hw_w = c.pre_highway_w ? f->dev + o.pre_hw : nullptr; d.hw = f->dev + o.hw;
        for (int i = 0; i < 2; ++i) { d.w_ih[i] = f->dev + o.w_ih[i]; d.b_ih[i] = f->dev + o.b_ih[i]; d.w_hh[i] = f->dev + o.w_hh[i]; d.b_hh[i] = f->dev + o.b_hh[i]; }
    };
    fill(f->enc, w->encoder_cbhg, oe);
    fill(f->post, w->postnet, op);
    *out = f;
    return WRNN_OK;
}

extern "C" void wrnn_taco_front_destroy(wrnn_taco_front *f)
{
    if (!f) return;
    if (f->dev) (void)hipFree(f->dev);
    delete f;
}

// workspace regions, each a multiple of 256 bytes: t0 [rows][w_t0], x [rows][w_x], bank [rows][w_bank], p2 [rows][w_x], ph [rows][128],
// hw [rows][128], gi [2][rows][384], ro [rows][256]
static size_t cb_region(size_t rows, size_t width) { return (rows * width * sizeof(float) + 255) / 256 * 256; }

extern "C" size_t wrnn_taco_front_workspace_bytes(const wrnn_taco_front *f, int32_t rows)
{
    if (!f || rows < 1) return 0;
    const size_t r = (size_t)rows;
    return cb_region(r, f->w_t0) + 2 * cb_region(r, f->w_x) + cb_region(r, f->w_bank) + 2 * cb_region(r, CB_C) + 2 * cb_region(r, 3 * CB_C) +
           cb_region(r, 2 * CB_C);
}

struct CbWs { float *t0, *x, *bank, *p2, *ph, *hw, *gi[2], *ro; };

static CbWs cb_carve(const wrnn_taco_front *f, void *workspace, size_t rows)
{
    char *p = (char *)workspace;
    CbWs s;
    s.t0 = (float *)p; p += cb_region(rows, f->w_t0);
    s.x = (float *)p; p += cb_region(rows, f->w_x);
    s.bank = (float *)p; p += cb_region(rows, f->w_bank);
    s.p2 = (float *)p; p += cb_region(rows, f->w_x);
    s.ph = (float *)p; p += cb_region(rows, CB_C);
    s.hw = (float *)p; p += cb_region(rows, CB_C);
    s.gi[0] = (float *)p; p += cb_region(rows, 3 * CB_C);
    s.gi[1] = (float *)p; p += cb_region(rows, 3 * CB_C);
    s.ro = (float *)p;
    return s;
}

static ConvArgs cb_linear(const float *in, int ldin, const float *w, const float *bias, float *out, int n, int K, int M, int flags)
{
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.in = in; a.w = w; a.bias = bias; a.out = out;
    a.n = n; a.Cin = K; a.Cout = M; a.taps = 1; a.ldin = ldin; a.ldo = M; a.flags = flags;
    return a;
}

enum CbKernel { CB_K_CONV, CB_K_ROWLIN, CB_K_BANK };

// One stage on a grid of (position tiles, gy, gz): the single-sentence kernel over a.n positions, or -- with a sentence table -- its _many twin over
// the concatenated tile list (a.in / a.ids / a.res / a.out are then the concatenated tensors and a.n is unused)
static void cb_launch(CbKernel k, const ConvArgs &a, unsigned gy, unsigned gz, const FrontTab *tab, hipStream_t stream)
{
    if (tab) {
        const dim3 grid((unsigned)tab->tile0[tab->n_sent], gy, gz);
        if (k == CB_K_BANK) hipLaunchKernelGGL(wrnn_cbhg_bank_many_kernel, grid, dim3(NT), 0, stream, a, *tab);
        else if (k == CB_K_CONV) hipLaunchKernelGGL(wrnn_cbhg_conv_many_kernel, grid, dim3(NT), 0, stream, a, *tab);
        else hipLaunchKernelGGL(wrnn_rowlin_many_kernel, grid, dim3(NT), 0, stream, a, *tab);
        return;
    }
    const dim3 grid((unsigned)((a.n + CB_NP - 1) / CB_NP), gy, gz);
    if (k == CB_K_BANK) hipLaunchKernelGGL(wrnn_cbhg_bank_kernel, grid, dim3(NT), 0, stream, a);
    else if (k == CB_K_CONV) hipLaunchKernelGGL(wrnn_cbhg_conv_kernel, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(wrnn_rowlin_kernel, grid, dim3(NT), 0, stream, a);
}

// One CBHG: x ([n][Cin] rows, or [Cin][n] with x_cmajor) -> gru_out [n][256]; pre_rnn (optional) receives the highway output.  With a sentence
// table n is the sum of the lengths, the row tensors are the concatenated ones and a [Cin][n_s] input is taken from the table's src[s].
static int cb_run_cbhg(const wrnn_taco_front *f, const CbhgDev &d, const float *x, bool x_cmajor, int n, const FrontTab *tab, const CbWs &s,
                       float *gru_out, float *pre_rnn, hipStream_t stream)
{
    ConvArgs a;
    memset(&a, 0, sizeof a);                                                // the bank: ReLU -> BatchNorm, all widths in one launch
    a.in = x; a.w = d.bank_w; a.scale = d.bank_ss; a.out = s.bank;
    a.n = n; a.Cin = d.Cin; a.Cout = CB_C; a.ldin = d.Cin; a.ldo = d.K * CB_C; a.flags = CB_RELU | (x_cmajor ? CB_IN_CMAJOR : 0);
    cb_launch(CB_K_BANK, a, CB_C / 16, d.K, tab, stream);
    memset(&a, 0, sizeof a);                                                // max-pool (in the loader) -> conv_project1 -> ReLU -> BatchNorm
    a.in = s.bank; a.w = d.p1_w; a.scale = d.p1_ss; a.shift = d.p1_ss + d.P1; a.out = s.t0;
    a.n = n; a.Cin = d.K * CB_C; a.Cout = d.P1; a.taps = 3; a.ldin = d.K * CB_C; a.ldo = d.P1; a.flags = CB_RELU | CB_POOL;
    cb_launch(CB_K_CONV, a, d.P1 / 16, 1, tab, stream);
    memset(&a, 0, sizeof a);                                                // conv_project2 -> BatchNorm -> + input
    a.in = s.t0; a.w = d.p2_w; a.scale = d.p2_ss; a.shift = d.p2_ss + d.P2; a.res = x; a.out = s.p2;
    a.n = n; a.Cin = d.P1; a.Cout = d.P2; a.taps = 3; a.ldin = d.P1; a.ldres = d.Cin; a.ldo = d.P2; a.flags = x_cmajor ? CB_RES_CMAJOR : 0;
    cb_launch(CB_K_CONV, a, d.P2 / 16, 1, tab, stream);
    const float *hin = s.p2;
    if (d.pre_hw_w) {
        a = cb_linear(s.p2, d.P2, d.pre_hw_w, nullptr, s.ph, n, d.P2, CB_C, 0);
        cb_launch(CB_K_ROWLIN, a, CB_C / 16, 1, tab, stream);
        hin = s.ph;
    }
    HighwayArgs hgw;
    hgw.in = hin; hgw.out = pre_rnn ? pre_rnn : s.hw; hgw.hw = d.hw; hgw.n = n; hgw.layers = d.layers;
    if (tab) hipLaunchKernelGGL(wrnn_highway_many_kernel, dim3((unsigned)tab->tile0[tab->n_sent]), dim3(NT), 0, stream, hgw, *tab);
    else hipLaunchKernelGGL(wrnn_highway_kernel, dim3((unsigned)((n + CB_NP - 1) / CB_NP)), dim3(NT), 0, stream, hgw);
    for (int dir = 0; dir < 2; ++dir) {
        a = cb_linear(hgw.out, CB_C, d.w_ih[dir], d.b_ih[dir], s.gi[dir], n, CB_C, 3 * CB_C, 0);
        cb_launch(CB_K_ROWLIN, a, 3 * CB_C / 16, 1, tab, stream);
    }
    CB_HIP(hipGetLastError());
    if (tab) {
        wrnn_bigru_many_call g;
        memset(&g, 0, sizeof g);
        g.struct_bytes = sizeof g;
        g.n_seq = tab->n_sent; g.hidden = CB_C; g.T = tab->n;
        g.gi_fwd = s.gi[0]; g.gi_rev = s.gi[1]; g.w_hh_fwd = d.w_hh[0]; g.w_hh_rev = d.w_hh[1]; g.b_hh_fwd = d.b_hh[0]; g.b_hh_rev = d.b_hh[1];
        g.out = gru_out; g.stream = (void *)stream;
        return wrnn_bigru_many(f->device, &g);
    }
    wrnn_bigru_call g;
    memset(&g, 0, sizeof g);
    g.struct_bytes = sizeof g;
    g.T = n; g.hidden = CB_C;
    g.gi_fwd = s.gi[0]; g.gi_rev = s.gi[1]; g.w_hh_fwd = d.w_hh[0]; g.w_hh_rev = d.w_hh[1]; g.b_hh_fwd = d.b_hh[0]; g.b_hh_rev = d.b_hh[1];
    g.out = gru_out; g.stream = (void *)stream;
    return wrnn_bigru(f->device, &g);
}

static int cb_check_call(const wrnn_taco_front *f, int32_t rows, const void *workspace, size_t workspace_bytes)
{
    if (rows < 1 || rows > (1 << 20)) CB_FAIL(WRNN_ERR_ARG, "bad length %d (1..%d)", rows, 1 << 20);
    if (workspace_bytes < wrnn_taco_front_workspace_bytes(f, rows)) CB_FAIL(WRNN_ERR_WORKSPACE, "workspace too small");
    if (((uintptr_t)workspace & 255) != 0) CB_FAIL(WRNN_ERR_ARG, "workspace must be 256-byte aligned");
    if (f->device < 0) CB_FAIL(WRNN_ERR_NO_DEVICE, "a dims-only handle (wrnn_taco_front_debug_host_handle) launches nothing");
    return WRNN_OK;
}

// ids -> seq_out, seq_proj_out over n rows: one sentence, or (tab) the concatenated rows of its sentences
static int cb_encode(const wrnn_taco_front *f, const int32_t *ids, int n, const FrontTab *tab, float *seq_out, float *seq_proj_out, float *pre_rnn_out,
                     void *workspace, hipStream_t stream)
{
    DeviceGuard dg(f->device);
    CB_HIP(dg.err);
    const CbWs s = cb_carve(f, workspace, (size_t)n);
    const int Cin = f->enc.Cin;
    ConvArgs a = cb_linear(f->emb, f->E, f->fc1_w, f->fc1_b, s.t0, n, f->E, f->PN1, CB_RELU);      // embedding rows -> fc1 -> ReLU
    a.ids = ids; a.table_rows = f->n_symbols;
    cb_launch(CB_K_ROWLIN, a, f->PN1 / 16, 1, tab, stream);
    a = cb_linear(s.t0, f->PN1, f->fc2_w, f->fc2_b, s.x, n, f->PN1, Cin, CB_RELU);
    cb_launch(CB_K_ROWLIN, a, Cin / 16, 1, tab, stream);
    const int rc = cb_run_cbhg(f, f->enc, s.x, false, n, tab, s, seq_out, pre_rnn_out, stream);
    if (rc != WRNN_OK) return rc;
    a = cb_linear(seq_out, 2 * CB_C, f->enc_proj_w, nullptr, seq_proj_out, n, 2 * CB_C, f->D, 0);
    cb_launch(CB_K_ROWLIN, a, f->D / 16, 1, tab, stream);
    CB_HIP(hipGetLastError());
    return WRNN_OK;
}

// mel ([n_mels][N]; with a table: src[s] of every sentence) -> linear_out over N rows
static int cb_postnet(const wrnn_taco_front *f, const float *mel, int N, const FrontTab *tab, float *linear_out, float *pre_rnn_out, void *workspace,
                      hipStream_t stream)
{
    DeviceGuard dg(f->device);
    CB_HIP(dg.err);
    const CbWs s = cb_carve(f, workspace, (size_t)N);
    const int rc = cb_run_cbhg(f, f->post, mel, true, N, tab, s, s.ro, pre_rnn_out, stream);
    if (rc != WRNN_OK) return rc;
    const ConvArgs a = cb_linear(s.ro, 2 * CB_C, f->post_proj_w, nullptr, linear_out, N, 2 * CB_C, f->fft, 0);
    cb_launch(CB_K_ROWLIN, a, f->fft / 16, 1, tab, stream);
    CB_HIP(hipGetLastError());
    return WRNN_OK;
}

extern "C" int wrnn_taco_encode(const wrnn_taco_front *f, const int32_t *ids, int32_t n, float *seq_out, float *seq_proj_out,
                                float *pre_rnn_out, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!f || !ids || !seq_out || !seq_proj_out || !workspace) CB_FAIL(WRNN_ERR_ARG, "NULL argument");
    if ((((uintptr_t)seq_out | (uintptr_t)seq_proj_out | (uintptr_t)pre_rnn_out) & 15) != 0) CB_FAIL(WRNN_ERR_ARG, "outputs must be 16-byte aligned");
    const int rc = cb_check_call(f, n, workspace, workspace_bytes);
    if (rc != WRNN_OK) return rc;
    return cb_encode(f, ids, n, nullptr, seq_out, seq_proj_out, pre_rnn_out, workspace, (hipStream_t)stream_);
}

extern "C" int wrnn_taco_postnet(const wrnn_taco_front *f, const float *mel, int32_t N, float *linear_out, float *pre_rnn_out,
                                 void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!f || !mel || !linear_out || !workspace) CB_FAIL(WRNN_ERR_ARG, "NULL argument");
    if ((((uintptr_t)linear_out | (uintptr_t)pre_rnn_out) & 15) != 0) CB_FAIL(WRNN_ERR_ARG, "outputs must be 16-byte aligned");
    const int rc = cb_check_call(f, N, workspace, workspace_bytes);
    if (rc != WRNN_OK) return rc;
    return cb_postnet(f, mel, N, nullptr, linear_out, pre_rnn_out, workspace, (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------------------------------------
// A list of sentences per call: the sentence table (FrontTab), built on the host and passed with every launch
// ---------------------------------------------------------------------------------------------------------
static bool cb_len_ok(int32_t n) { return n >= 1 && n <= (1 << 20); }

extern "C" size_t wrnn_taco_front_workspace_bytes_many(const wrnn_taco_front *f, const int32_t *n, int32_t n_sent)
{
    if (!f || !n || n_sent < 1 || n_sent > CB_MANY) return 0;
    int32_t rows = 0;                                                       // <= 64 * 2^20
    for (int s = 0; s < n_sent; ++s) {
        if (!cb_len_ok(n[s])) return 0;
        rows += n[s];
    }
    return wrnn_taco_front_workspace_bytes(f, rows);                        // the regions of the single call, over the concatenated rows
}

// the table of a call and its row count; `src`: NULL, or the per-sentence [n_mels][N_s] inputs
static int cb_table(const int32_t *n, int32_t n_sent, const float *const *src, FrontTab *t, int *rows)
{
    if (!n) CB_FAIL(WRNN_ERR_ARG, "NULL length table");
    if (n_sent < 1 || n_sent > CB_MANY) CB_FAIL(WRNN_ERR_ARG, "bad sentence count %d (1..%d per call)", n_sent, CB_MANY);
    memset(t, 0, sizeof *t);
    t->n_sent = n_sent;
    int row = 0, tile = 0;
    for (int s = 0; s < n_sent; ++s) {
        if (!cb_len_ok(n[s])) CB_FAIL(WRNN_ERR_ARG, "sentence %d: bad length %d (1..%d)", s, n[s], 1 << 20);
        if (src && !src[s]) CB_FAIL(WRNN_ERR_ARG, "sentence %d: NULL mel", s);
        t->n[s] = n[s]; t->row0[s] = row; t->tile0[s] = tile;
        if (src) t->src[s] = src[s];
        row += n[s];
        tile += (n[s] + CB_NP - 1) / CB_NP;
    }
    t->tile0[n_sent] = tile;
    *rows = row;
    return WRNN_OK;
}

static int cb_check_call_many(const wrnn_taco_front *f, const int32_t *n, int32_t n_sent, const void *workspace, size_t workspace_bytes)
{
    if (((uintptr_t)workspace & 255) != 0) CB_FAIL(WRNN_ERR_ARG, "workspace must be 256-byte aligned");
    const size_t need = wrnn_taco_front_workspace_bytes_many(f, n, n_sent);
    if (workspace_bytes < need) CB_FAIL(WRNN_ERR_WORKSPACE, "workspace too small: %zu bytes, wrnn_taco_front_workspace_bytes_many says %zu", workspace_bytes, need);
    if (f->device < 0) CB_FAIL(WRNN_ERR_NO_DEVICE, "a dims-only handle (wrnn_taco_front_debug_host_handle) launches nothing");
    return WRNN_OK;
}

extern "C" int wrnn_taco_encode_many(const wrnn_taco_front *f, const int32_t *ids, const int32_t *n, int32_t n_sent, float *seq_out,
                                     float *seq_proj_out, float *pre_rnn_out, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!f || !ids || !seq_out || !seq_proj_out || !workspace) CB_FAIL(WRNN_ERR_ARG, "NULL argument");
    FrontTab tab;
    int rows = 0;
    int rc = cb_table(n, n_sent, nullptr, &tab, &rows);
    if (rc != WRNN_OK) return rc;
    if ((((uintptr_t)seq_out | (uintptr_t)seq_proj_out | (uintptr_t)pre_rnn_out) & 15) != 0) CB_FAIL(WRNN_ERR_ARG, "outputs must be 16-byte aligned");
    rc = cb_check_call_many(f, n, n_sent, workspace, workspace_bytes);
    if (rc != WRNN_OK) return rc;
    return cb_encode(f, ids, rows, &tab, seq_out, seq_proj_out, pre_rnn_out, workspace, (hipStream_t)stream_);
}

extern "C" int wrnn_taco_postnet_many(const wrnn_taco_front *f, const float *const *mel, const int32_t *N, int32_t n_sent, float *linear_out,
                                      float *pre_rnn_out, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!f || !linear_out || !workspace) CB_FAIL(WRNN_ERR_ARG, "NULL argument");
    if (!mel) CB_FAIL(WRNN_ERR_ARG, "NULL mel table");
    FrontTab tab;
    int rows = 0;
    int rc = cb_table(N, n_sent, mel, &tab, &rows);
    if (rc != WRNN_OK) return rc;
    if ((((uintptr_t)linear_out | (uintptr_t)pre_rnn_out) & 15) != 0) CB_FAIL(WRNN_ERR_ARG, "outputs must be 16-byte aligned");
    rc = cb_check_call_many(f, N, n_sent, workspace, workspace_bytes);
    if (rc != WRNN_OK) return rc;
    return cb_postnet(f, tab.src[0], rows, &tab, linear_out, pre_rnn_out, workspace, (hipStream_t)stream_);
}
