// wrnn_abi.hip -- host side of the C ABI declared in include/wavernn_amd.h.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>

#include "../../include/wavernn_amd.h"
#include "wrnn_device.h"

namespace wrnn {
hipError_t launch_cond(const CondArgs &a, int n_cus, bool valu, hipStream_t stream);
hipError_t launch_cond_frames(const CondArgs &a, hipStream_t stream);
hipError_t launch_cond_frames_slab(const CondArgs &a, hipStream_t stream);
hipError_t launch_slab_prep(const CondArgs &a, const float *nz_in, float *nz_out, long nz_n, unsigned *xcc, int n_cus, hipStream_t stream);
hipError_t launch_cond_frag(const CondArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_noise_mol(const float *in, float *out, long n, int B, int n_cus, hipStream_t stream);
hipError_t launch_noise_fill(bool mol, int B, int C, int t0, int t1, uint64_t seed, const uint64_t *seg_id, float *out, int n_cus, hipStream_t stream);
void noise_fill_host(bool mol, int B, int C, int t0, int t1, uint64_t seed, const uint64_t *seg_id, float *out);
struct NllArgs { const float *logits, *target; const int *seg_len; float *nll; double *sum; int n, T, C; };      // (csrc/wrnn_nll.hip)
hipError_t launch_nll(bool mol, const NllArgs &a, hipStream_t stream);
void nll_host(bool mol, const NllArgs &a);
hipError_t launch_stream(const LoopArgs &args, int mode, hipStream_t stream);
hipError_t launch_loop(const LoopArgs &args, int ncl, int mode, hipStream_t stream);
int loop_max_depth(int mode);
size_t loop_state_floats(int G);
hipError_t launch_generic(const GenArgs &args, int mode, hipStream_t stream);
bool generic_dims_ok(int H, int F, int M, int A, int C, int mode);
hipError_t launch_tile(const GenArgs &args, int mode, hipStream_t stream);
size_t tile_lds_bytes(int H, int F, int M, int A, int C);
bool tile_dims_ok(int H, int F, int M, int A, int C, int mode);
hipError_t launch_tile_wide(const GenArgs &args, int mode, int W, void *xws, unsigned *status, hipStream_t stream);
size_t tile_wide_flag_bytes(int tiles);
size_t tile_wide_xbuf_bytes(int tiles, int H, int F, int C, int mode);
hipError_t launch_tile_sparse(const GenArgs &args, const TileSparseArgs &sp, int mode, bool fcs, hipStream_t stream);
hipError_t launch_tile_bf16(const GenArgs &args, const TileBf16Args &bw, int mode, hipStream_t stream);
hipError_t launch_duo(const LoopArgs &args, int ncl, int mode, hipStream_t stream);
int duo_max_depth();
size_t duo_xbuf_bytes(int G);
size_t duo_xbuf_bytes_max();
hipError_t launch_sparse(const LoopArgs &args, int nbp, int mode, hipStream_t stream);
int sparse_clusters(int n_cus);
int sparse_max_slots();
size_t sparse_state_floats(int slots);
size_t sparse_xbuf_bytes(int slots);
hipError_t launch_put_floats(float *dst, const float *src, int n, hipStream_t stream);
hipError_t launch_chain(const LoopArgs &args, int mode, hipStream_t stream);
hipError_t launch_octo(const LoopArgs &args, int ncl, int mode, hipStream_t stream);
int octo_max_depth();
int chain_clusters(int n_cus);
int chain_max_depth();
size_t chain_state_floats(int G);
size_t chain_xbuf_bytes(int G);
int selftest_mfma(char *msg, size_t n);
int selftest_allgather(int n_cus, char *msg, size_t n, float *us_per_round);
int selftest_tanh(char *msg, size_t n);
int selftest_xor(char *msg, size_t n);
}  // namespace wrnn

using namespace wrnn;

static thread_local char g_err[512] = "";
static void set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return WRNN_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

struct wrnn_pack {
    int device;
    wrnn_plan_traits tr;       // everything the launch planner reads (make_plan, ws_layout): n_cus, mode, C, generic + dims, sp_nbp, sp_max_blocks
    size_t weight_bytes;
    char *dev;          // one allocation
    size_t dev_bytes;
    // device pointers into `dev`
    const float *I_w0, *I_b, *I_cT;
    const float *w_ih1, *w_hh1, *b_ih1, *b_hh1, *w_ih2, *w_hh2, *b_ih2, *b_hh2;
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *fc3_w, *fc3_b;
    const float *w_ih1T, *w_hh1T, *w_ih2T, *w_hh2T, *fc1T, *fc2T, *fc3T, *c2_wT, *c3_wT, *c4_wT;
    const float *fc3f;         // MOL: fc3.weight in A-fragment order (wrnn_duo.hip)
    const float *u1;           // MOL: rnn1.weight_ih . I.weight[:,0] [3H] -- the x_{t-1} term of rnn1's gi (wrnn_duo.hip)
    // dimension-generic pack (any hparams but the shipped ones): only the k-major copies + biases, run by wrnn_generic_kernel
    const float *g_I_T, *g_fc1T, *g_fc2T, *g_w_ih2T;      // (the other k-major copies are the fields above)
    // ... and its tile-sparse view (wrnn_tile_sparse.hip): 0 none, 1 the four GRU matrices, 2 fc1 / fc2 too; surviving / all 16x1 blocks of w_ih1, w_hh1, w_ih2,
    // w_hh2, fc1, fc2 (0 / 0: the matrix's row count is no multiple of 16, nothing was counted)
    int ts_view;
    int32_t ts_kept[6], ts_total[6];
    TileSparseArgs ts;
    // ... and its bf16 view (wrnn_tile_bf16.hip): the eight matrices rounded to bfloat16; bf_bytes == 0: none
    size_t bf_bytes;
    TileBf16Args bf;
    const float *sp_vals;
    const int *sp_cols;
    int sp_fc_max_blocks;      // fc1 / fc2 (columns [0, H): the aux columns live in the per-frame tables): largest block row
    const float *sp_fc_vals;   // non-null: the Linear layers are block-sparse too (the notebook prunes them as well) -> wrnn_sparse_kernel's gathered fc stages
    const int *sp_fc_cols;
};

extern "C" const char *wrnn_last_error(void) { return g_err; }
extern "C" int wrnn_abi_version(void) { return WRNN_ABI_VERSION; }

extern "C" int wrnn_device_cus(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) {
        set_err("no HIP device %d (count %d)", device, n);
        return WRNN_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return WRNN_ERR_NO_DEVICE;
    return prop.multiProcessorCount;
}

namespace {
struct Builder {
    std::vector<float> host;
    size_t add(const float *src, size_t n)
    {
        size_t off = (host.size() + 63) / 64 * 64;   // 256-byte alignment
        host.resize(off + n);
        if (src) memcpy(host.data() + off, src, n * sizeof(float));
        return off;
    }
    // dst[k][r] = src[r][col0 + k], src is [rows][ld]
    size_t add_T(const float *src, int rows, int ld, int col0, int ncols)
    {
        size_t off = add(nullptr, (size_t)ncols * rows);
        float *d = host.data() + off;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < ncols; ++k) d[(size_t)k * rows + r] = src[(size_t)r * ld + col0 + k];
        return off;
    }
};

// The tile-sparse view of one matrix W [rows][K] (row-major, rows a multiple of 16): the layout of TileSparseMat (wrnn_device.h).  Host only.
struct TileSparsePacked {
    std::vector<int32_t> tab, cols;     // [rows / 16][2], [groups][16]
    std::vector<float> vals;            // [groups][64][4]
    int kept, total;                    // surviving / all 16x1 blocks
};
void tile_sparse_pack(const float *W, int rows, int K, TileSparsePacked &o)
{
    const int nbr = rows / 16;
    o.tab.assign((size_t)2 * nbr, 0); o.cols.clear(); o.vals.clear();
    o.kept = 0; o.total = nbr * K;
    std::vector<int> cv;
    for (int br = 0; br < nbr; ++br) {
        const float *base = W + (size_t)16 * br * K;
        cv.clear();
        for (int c = 0; c < K; ++c) {
            bool nz = false;
            for (int r = 0; r < 16 && !nz; ++r) nz = base[(size_t)r * K + c] != 0.0f;
            if (nz) cv.push_back(c);
        }
        const int n = (int)cv.size(), ng = (n + 15) / 16, g0 = (int)(o.cols.size() / 16);
        o.kept += n;
        o.tab[2 * br] = g0; o.tab[2 * br + 1] = n;
        o.cols.resize((size_t)(g0 + ng) * 16);
        o.vals.resize((size_t)(g0 + ng) * 256);
        for (int g = 0; g < ng; ++g)
            for (int kq = 0; kq < 4; ++kq)
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * g + 4 * e + kq;                  // list entry; past the list: padding = value 0 at the last surviving column
                    const int c = k < n ? cv[k] : cv[n - 1];
                    o.cols[((size_t)(g0 + g) * 4 + kq) * 4 + e] = c;
                    for (int i = 0; i < 16; ++i) o.vals[(((size_t)(g0 + g) * 64) + 16 * kq + i) * 4 + e] = k < n ? base[(size_t)i * K + c] : 0.0f;
                }
    }
}
// a view needs at most 41 % of a matrix's blocks to survive (include/wavernn_amd.h, WRNN_ALGO_TILE_SPARSE): the 60 % sparsity level of `prune.block_mask`, whose
// per-gate rounding keeps 40.01 %, is the least sparse one at which wrnn_tile_sparse_kernel measured no slower than wrnn_tile_kernel (profiles/tile_sparse_ab.json:
// 91.8 vs 92.6 us per step; at 50 % it is 0.87 x)
bool tile_sparse_admits(int kept, int total) { return total > 0 && 100 * (long)kept <= 41 * (long)total; }

// The bf16 image of one matrix W [rows][K] (row-major): the layout wrnn_tile_bf16.hip describes -- [k / 32][row][k % 4][(k % 32) / 4], the weights rounded to
// bfloat16 round-to-nearest-even, k >= K and the 64 rows behind the last k-step +0.  false: a value is not finite, or rounds to +-inf.  Host only.
constexpr int BF16_TAIL_ROWS = 64;
bool tile_bf16_pack(const float *W, int rows, int K, std::vector<uint16_t> &o)
{
    const int nsteps = (K + 31) / 32;
    o.assign(((size_t)nsteps * rows + BF16_TAIL_ROWS) * 32, 0);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < K; ++k) {
            uint32_t u;
            memcpy(&u, W + (size_t)r * K + k, sizeof u);
            if ((u & 0x7F800000u) == 0x7F800000u) return false;
            const uint32_t q = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
            if ((q & 0x7F80u) == 0x7F80u) return false;
            o[(((size_t)(k >> 5) * rows + r) * 4 + (k & 3)) * 8 + ((k & 31) >> 2)] = (uint16_t)q;
        }
    return true;
}
}  // namespace

extern "C" int wrnn_debug_tile_bf16_pack(const float *W, int32_t rows, int32_t K, uint16_t *out, size_t cap)
{
    if (!W || rows < 1 || K < 1) { set_err("bad argument"); return WRNN_ERR_ARG; }
    if (((size_t)(K + 31) / 32 * rows + BF16_TAIL_ROWS) * 32 > 0x7FFFFFFFu) { set_err("%d x %d: more than 2^31 elements", rows, K); return WRNN_ERR_ARG; }
    std::vector<uint16_t> img;
    if (!tile_bf16_pack(W, rows, K, img)) {
        set_err("a weight is not finite or rounds to +-inf in bfloat16 (its magnitude is above 3.3895e38): no bf16 image");
        return WRNN_ERR_ARG;
    }
    if (out && img.size() <= cap) memcpy(out, img.data(), img.size() * sizeof(uint16_t));
    return (int)img.size();
}

extern "C" int wrnn_debug_tile_sparse_pack(const float *W, int32_t rows, int32_t K, int32_t gates, int32_t *tab, int32_t *cols, float *vals,
                                           int32_t group_capacity, int32_t *kept, int32_t *total, int32_t *admitted)
{
    if (!W || !tab || !kept || !total || !admitted || rows < 1 || K < 1 || gates < 1 || rows % gates) { set_err("bad argument"); return WRNN_ERR_ARG; }
    if ((rows / gates) % 16) { set_err("%d rows per gate: no multiple of 16", rows / gates); return WRNN_ERR_ARG; }
    TileSparsePacked pk;
    tile_sparse_pack(W, rows, K, pk);
    const int groups = (int)(pk.cols.size() / 16);
    memcpy(tab, pk.tab.data(), pk.tab.size() * sizeof(int32_t));
    *kept = pk.kept; *total = pk.total; *admitted = tile_sparse_admits(pk.kept, pk.total) ? 1 : 0;
    if (cols && vals && groups <= group_capacity) {
        memcpy(cols, pk.cols.data(), pk.cols.size() * sizeof(int32_t));
        memcpy(vals, pk.vals.data(), pk.vals.size() * sizeof(float));
    }
    return groups;
}

extern "C" int wrnn_pack_create(const wrnn_weights *w, int device, wrnn_pack **out)
{
    if (!w || !out) { set_err("NULL argument"); return WRNN_ERR_ARG; }
    const int C = w->n_classes;
    // the shipped geometry -- what the MFMA kernels and the stream kernel are built for; RAW with more classes than the stream kernel has threads
    // (bits > 9) takes the generic pack like any other non-shipped hparam
    const bool shipped = w->rnn_dims == H && w->fc_dims == H && w->feat_dims == MEL && w->aux_dims == AUX && !(w->mode == WRNN_MODE_RAW && C > H);
    if (w->mode == WRNN_MODE_MOL) {
        if (C != 30) { set_err("MOL needs n_classes == 30"); return WRNN_ERR_ARG; }
    } else if (w->mode == WRNN_MODE_RAW) {
        if (shipped && C < 2) { set_err("RAW needs 2 <= n_classes <= 2048 (the shipped dims: up to 512 on the MFMA / stream kernels, more on the generic kernel)"); return WRNN_ERR_ARG; }
    } else { set_err("unknown mode %d", w->mode); return WRNN_ERR_ARG; }
    if (!shipped && !generic_dims_ok(w->rnn_dims, w->fc_dims, w->feat_dims, w->aux_dims, C, w->mode)) {
        set_err("unsupported dims rnn=%d fc=%d feat=%d aux=%d classes=%d: the generic kernel takes rnn, fc, classes <= 2048, feat + aux <= 1024 "
                "(MOL: 30 classes)", w->rnn_dims, w->fc_dims, w->feat_dims, w->aux_dims, C);
        return WRNN_ERR_ARG;
    }
    const float *const *ptrs = &w->I_w;
    for (int i = 0; i < 16; ++i)
        if (!ptrs[i]) { set_err("NULL weight pointer #%d", i); return WRNN_ERR_ARG; }
    const int cus = wrnn_device_cus(device);
    if (cus < 0) return cus;
    DeviceGuard dg(device);
    HIPCHK(dg.err);

    if (!shipped) {
        // ---- generic pack: k-major copies of the eight matrices + the biases (wrnn_generic.hip reads nothing else)
        const int gH = w->rnn_dims, gF = w->fc_dims, gM = w->feat_dims, gA = w->aux_dims;
        Builder b;
        const size_t oI = b.add_T(w->I_w, gH, 1 + gM + gA, 0, 1 + gM + gA), oIb = b.add(w->I_b, gH);
        const size_t o1i = b.add_T(w->w_ih1, 3 * gH, gH, 0, gH), o1h = b.add_T(w->w_hh1, 3 * gH, gH, 0, gH);
        const size_t o1bi = b.add(w->b_ih1, 3 * gH), o1bh = b.add(w->b_hh1, 3 * gH);
        const size_t o2i = b.add_T(w->w_ih2, 3 * gH, gH + gA, 0, gH + gA), o2h = b.add_T(w->w_hh2, 3 * gH, gH, 0, gH);
        const size_t o2bi = b.add(w->b_ih2, 3 * gH), o2bh = b.add(w->b_hh2, 3 * gH);
        const size_t of1 = b.add_T(w->fc1_w, gF, gH + gA, 0, gH + gA), of1b = b.add(w->fc1_b, gF);
        const size_t of2 = b.add_T(w->fc2_w, gF, gF + gA, 0, gF + gA), of2b = b.add(w->fc2_b, gF);
        const size_t of3 = b.add_T(w->fc3_w, C, gF, 0, gF), of3b = b.add(w->fc3_b, C);
        // ---- the tile-sparse view (wrnn_tile_sparse.hip): the GRU matrices when rnn % 16 == 0 and at most 41 % of the blocks of each survive (tile_sparse_admits); fc1 / fc2 in
        // addition when fc % 16 == 0 and the same holds for both.  The dense copies above stay: `tile` and `auto` run the pack as before
        const float *ts_src[6] = {w->w_ih1, w->w_hh1, w->w_ih2, w->w_hh2, w->fc1_w, w->fc2_w};
        const int ts_rows[6] = {3 * gH, 3 * gH, 3 * gH, 3 * gH, gF, gF}, ts_K[6] = {gH, gH, gH + gA, gH, gH + gA, gF + gA};
        TileSparsePacked ts_pk[6];
        int32_t ts_kept[6] = {0}, ts_total[6] = {0};
        size_t ts_off[6][3] = {{0}};
        bool gru_ok = gH % 16 == 0, fc_ok = gF % 16 == 0;
        for (int m = 0; m < 6; ++m) {
            if (m < 4 ? gH % 16 : gF % 16) continue;
            tile_sparse_pack(ts_src[m], ts_rows[m], ts_K[m], ts_pk[m]);
            ts_kept[m] = ts_pk[m].kept; ts_total[m] = ts_pk[m].total;
            if (!tile_sparse_admits(ts_kept[m], ts_total[m])) (m < 4 ? gru_ok : fc_ok) = false;
        }
        const int ts_view = !gru_ok ? 0 : fc_ok ? 2 : 1;
        for (int m = 0; m < (ts_view == 2 ? 6 : ts_view == 1 ? 4 : 0); ++m) {      // (ints stored in the float builder: same width)
            ts_off[m][0] = b.add(ts_pk[m].vals.data(), ts_pk[m].vals.size());
            ts_off[m][1] = b.add(reinterpret_cast<const float *>(ts_pk[m].cols.data()), ts_pk[m].cols.size());
            ts_off[m][2] = b.add(reinterpret_cast<const float *>(ts_pk[m].tab.data()), ts_pk[m].tab.size());
        }
        // ---- the bf16 view (wrnn_tile_bf16.hip): every pack whose dims pass wrnn_tile_kernel's LDS rule, unless a weight rounds to +-inf
        const float *bf_src[8] = {w->I_w, w->w_ih1, w->w_hh1, w->w_ih2, w->w_hh2, w->fc1_w, w->fc2_w, w->fc3_w};
        const int bf_rows[8] = {gH, 3 * gH, 3 * gH, 3 * gH, 3 * gH, gF, gF, C}, bf_K[8] = {1 + gM + gA, gH, gH, gH + gA, gH, gH + gA, gF + gA, gF};
        static const char *const bf_names[8] = {"I.weight", "rnn1.weight_ih", "rnn1.weight_hh", "rnn2.weight_ih", "rnn2.weight_hh", "fc1.weight", "fc2.weight", "fc3.weight"};
        size_t bf_off[8] = {0}, bf_bytes = 0;
        bool bf_view = tile_dims_ok(gH, gF, gM, gA, C, w->mode), bf_inf = false;
        for (int m = 0; m < 8 && bf_view; ++m) {      // (uint16 pairs stored in the float builder; an image is a whole number of 64-byte rows)
            std::vector<uint16_t> img;
            if (!tile_bf16_pack(bf_src[m], bf_rows[m], bf_K[m], img)) {
                // not an error: the pack runs on every other kernel.  The text is what wrnn_last_error() answers after this call
                set_err("wrnn_pack_create: no bf16 view -- a value of %s is not finite or rounds to +-inf in bfloat16; algo tile_bf16 will refuse this pack", bf_names[m]);
                bf_view = false; bf_inf = true; bf_bytes = 0;
                break;
            }
            bf_off[m] = b.add(reinterpret_cast<const float *>(img.data()), img.size() / 2);
            bf_bytes += img.size() * sizeof(uint16_t);
        }
        b.add(nullptr, 64);
        wrnn_pack *p = new wrnn_pack();
        memset(p, 0, sizeof *p);
        p->device = device; p->tr.n_cus = cus; p->tr.C = C; p->tr.mode = w->mode; p->tr.generic = 1;
        p->tr.gH = gH; p->tr.gF = gF; p->tr.gM = gM; p->tr.gA = gA;
        p->dev_bytes = b.host.size() * sizeof(float);
        p->weight_bytes = sizeof(float) * ((size_t)gH * (1 + gM + gA) + gH + 2 * ((size_t)3 * gH * gH) + (size_t)3 * gH * (gH + gA) + (size_t)3 * gH * gH +
                                           4 * 3 * gH + (size_t)gF * (gH + gA) + (size_t)gF * (gF + gA) + 2 * gF + (size_t)C * gF + C);
        hipError_t e = hipMalloc((void **)&p->dev, p->dev_bytes);
        if (e != hipSuccess) { set_err("hipMalloc(%zu) failed: %s", p->dev_bytes, hipGetErrorString(e)); delete p; return WRNN_ERR_HIP; }
        e = hipMemcpy(p->dev, b.host.data(), p->dev_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_err("hipMemcpy failed: %s", hipGetErrorString(e)); (void)hipFree(p->dev); delete p; return WRNN_ERR_HIP; }
        const float *base = (const float *)p->dev;
        p->g_I_T = base + oI; p->I_b = base + oIb;
        p->w_ih1T = base + o1i; p->w_hh1T = base + o1h; p->b_ih1 = base + o1bi; p->b_hh1 = base + o1bh;
        p->g_w_ih2T = base + o2i; p->w_hh2T = base + o2h; p->b_ih2 = base + o2bi; p->b_hh2 = base + o2bh;
        p->g_fc1T = base + of1; p->fc1_b = base + of1b; p->g_fc2T = base + of2; p->fc2_b = base + of2b;
        p->fc3T = base + of3; p->fc3_b = base + of3b;
        p->tr.sp_max_blocks = gH;
        p->ts_view = ts_view;
        for (int m = 0; m < 6; ++m) {
            p->ts_kept[m] = ts_kept[m]; p->ts_total[m] = ts_total[m];
            if (m < (ts_view == 2 ? 6 : ts_view == 1 ? 4 : 0))
                p->ts.m[m] = TileSparseMat{base + ts_off[m][0], reinterpret_cast<const int *>(base + ts_off[m][1]), reinterpret_cast<const int *>(base + ts_off[m][2])};
        }
        // what the planner reads of it (wrnn_plan_traits of a GENERIC pack): sp_nbp > 0 a view, sp_fc its fc half; sp_nbp < 0 names the first matrix that
        // keeps too many of its blocks, -(1 + 1001 m + its surviving fraction in 1/1000, rounded up)
        p->tr.sp_nbp = ts_view ? 1 : 0; p->tr.sp_fc = ts_view == 2 ? 1 : 0;
        // the bf16 view: the planner derives it from the dims (tile_dims_ok); bit 1 of sp_fc says that it is missing all the same
        p->bf_bytes = bf_view ? bf_bytes : 0;
        for (int m = 0; m < 8 && bf_view; ++m) p->bf.m[m] = reinterpret_cast<const uint16_t *>(base + bf_off[m]);
        if (bf_inf) p->tr.sp_fc |= 2;
        for (int m = 0; m < 4 && !ts_view && gH % 16 == 0; ++m)
            if (!tile_sparse_admits(ts_kept[m], ts_total[m])) {
                p->tr.sp_nbp = -(1 + 1001 * m + (int)(((long)ts_kept[m] * 1000 + ts_total[m] - 1) / ts_total[m]));
                break;
            }
        p->tr.struct_bytes = (int32_t)sizeof p->tr;
        *out = p;
        return WRNN_OK;
    }

    const int KI = 1 + MEL + AUX, K2 = H + AUX;
    Builder b;
    std::vector<float> col0(H);
    for (int r = 0; r < H; ++r) col0[r] = w->I_w[(size_t)r * KI];
    const size_t o_I_w0 = b.add(col0.data(), H), o_I_b = b.add(w->I_b, H);
    const size_t o_I_cT = b.add_T(w->I_w, H, KI, 1, KCOND);
    const size_t o_w_ih1 = b.add(w->w_ih1, (size_t)3 * H * H), o_w_hh1 = b.add(w->w_hh1, (size_t)3 * H * H);
    const size_t o_b_ih1 = b.add(w->b_ih1, 3 * H), o_b_hh1 = b.add(w->b_hh1, 3 * H);
    const size_t o_w_ih2 = b.add(w->w_ih2, (size_t)3 * H * K2), o_w_hh2 = b.add(w->w_hh2, (size_t)3 * H * H);
    const size_t o_b_ih2 = b.add(w->b_ih2, 3 * H), o_b_hh2 = b.add(w->b_hh2, 3 * H);
    const size_t o_fc1_w = b.add(w->fc1_w, (size_t)H * K2), o_fc1_b = b.add(w->fc1_b, H);
    const size_t o_fc2_w = b.add(w->fc2_w, (size_t)H * K2), o_fc2_b = b.add(w->fc2_b, H);
    const size_t o_fc3_w = b.add(w->fc3_w, (size_t)C * H), o_fc3_b = b.add(w->fc3_b, C);
    const size_t o_w_ih1T = b.add_T(w->w_ih1, 3 * H, H, 0, H), o_w_hh1T = b.add_T(w->w_hh1, 3 * H, H, 0, H);
    const size_t o_w_ih2T = b.add_T(w->w_ih2, 3 * H, K2, 0, H), o_w_hh2T = b.add_T(w->w_hh2, 3 * H, H, 0, H);
    const size_t o_fc1T = b.add_T(w->fc1_w, H, K2, 0, H), o_fc2T = b.add_T(w->fc2_w, H, K2, 0, H);
    const size_t o_fc3T = b.add_T(w->fc3_w, C, H, 0, H);
    const size_t o_c2_wT = b.add_T(w->w_ih2, 3 * H, K2, H, AUX);
    const size_t o_c3_wT = b.add_T(w->fc1_w, H, K2, H, AUX), o_c4_wT = b.add_T(w->fc2_w, H, K2, H, AUX);
    // MOL: fc3 (30 x 512) as two 16-row MFMA A tiles in fragment order: [tile][wave][k-block r][lane (row fi, k-quad kq)][4]
    // = fc3_w[16 tile + fi][128 wave + 16 r + 4 kq ..], rows >= 30 zero
    size_t o_fc3f = 0;
    if (w->mode == WRNN_MODE_MOL) {
        o_fc3f = b.add(nullptr, (size_t)2 * SEG * H);
        for (int q = 0; q < 2 * SEG * H / 4; ++q) {
            const int l6 = q & 63, r = (q >> 6) & 7, wv = (q >> 9) & 3, tile = q >> 11;
            const int row = 16 * tile + (l6 & 15), kq = l6 >> 4;
            for (int e = 0; e < 4; ++e)
                b.host[o_fc3f + (size_t)q * 4 + e] = row < C ? w->fc3_w[(size_t)row * H + 128 * wv + 16 * r + 4 * kq + e] : 0.f;
        }
    }
    // u1 = rnn1.weight_ih . I.weight[:,0] (double accumulation, rounded once): gi = W_ih . (cI + w0 x) + b = W_ih . cI + x u1 + b
    size_t o_u1 = 0;
    {
        o_u1 = b.add(nullptr, (size_t)3 * H);
        for (int r = 0; r < 3 * H; ++r) {
            double acc = 0.0;
            for (int k = 0; k < H; ++k) acc += (double)w->w_ih1[(size_t)r * H + k] * (double)col0[k];
            b.host[o_u1 + r] = (float)acc;
        }
    }
    // ---- block-sparse view of the GRU matrices (16x1 blocks: 16 consecutive rows of one gate x 1 column) -----------
    // usable by wrnn_sparse_kernel when every block row keeps <= 64 columns (~5 % density keeps ~26 +- 5), for MOL and for 9-bit RAW (512 classes)
    int sp_nbp = 0, sp_max = 0, sp_fc_max = 0;
    bool sp_fc_ok = false;
    size_t o_spv = 0, o_spc = 0, o_sfv = 0, o_sfc = 0;
    {
        const float *mats[4] = {w->w_ih1, w->w_hh1, w->w_ih2, w->w_hh2};
        const int lds_[4] = {H, H, K2, H};
        std::vector<std::vector<int>> cols((size_t)4 * 32 * 3);
        for (int m = 0; m < 4; ++m)
            for (int wg = 0; wg < 32; ++wg)
                for (int g = 0; g < 3; ++g) {
                    std::vector<int> &cv = cols[((size_t)m * 32 + wg) * 3 + g];
                    const float *base = mats[m] + ((size_t)g * H + 16 * wg) * lds_[m];
                    for (int c = 0; c < H; ++c) {
                        bool nz = false;
                        for (int r = 0; r < 16 && !nz; ++r) nz = base[(size_t)r * lds_[m] + c] != 0.0f;
                        if (nz) cv.push_back(c);
                    }
                    if ((int)cv.size() > sp_max) sp_max = (int)cv.size();
                }
        // fc1 / fc2 (round 6; "Pruning - Scratchpad.ipynb" :199-204 prunes the Linear layers too): their first H columns, 32 block rows each
        const float *fmats[2] = {w->fc1_w, w->fc2_w};
        std::vector<std::vector<int>> fcols((size_t)2 * 32);
        for (int m = 0; m < 2; ++m)
            for (int wg = 0; wg < 32; ++wg) {
                std::vector<int> &cv = fcols[(size_t)m * 32 + wg];
                const float *base = fmats[m] + (size_t)(16 * wg) * K2;
                for (int c = 0; c < H; ++c) {
                    bool nz = false;
                    for (int r = 0; r < 16 && !nz; ++r) nz = base[(size_t)r * K2 + c] != 0.0f;
                    if (nz) cv.push_back(c);
                }
                if ((int)cv.size() > sp_fc_max) sp_fc_max = (int)cv.size();
            }
        if (sp_max <= 64 && (w->mode == WRNN_MODE_MOL || C == H)) {
            sp_nbp = sp_max <= 48 ? 48 : 64;
            if (sp_fc_max <= 64) {                        // one NBP for the gate and the fc tiles of a launch
                if (sp_fc_max > 48) sp_nbp = 64;
                o_sfv = b.add(nullptr, (size_t)2 * 32 * sp_nbp * 16);
                o_sfc = b.add(nullptr, (size_t)2 * 32 * sp_nbp);
                for (size_t q = 0; q < (size_t)2 * 32 * sp_nbp * 16; ++q) b.host[o_sfv + q] = 0.f;
                int *fi_ = reinterpret_cast<int *>(b.host.data() + o_sfc);
                for (size_t q = 0; q < (size_t)2 * 32 * sp_nbp; ++q) fi_[q] = 0;
                for (int m = 0; m < 2; ++m)
                    for (int wg = 0; wg < 32; ++wg) {
                        const size_t br = (size_t)m * 32 + wg;
                        const std::vector<int> &cv = fcols[br];
                        const float *base = fmats[m] + (size_t)(16 * wg) * K2;
                        for (size_t k = 0; k < cv.size(); ++k) {
                            reinterpret_cast<int *>(b.host.data() + o_sfc)[br * sp_nbp + k] = cv[k];
                            for (int r = 0; r < 16; ++r) b.host[o_sfv + (br * sp_nbp + k) * 16 + r] = base[(size_t)r * K2 + cv[k]];
                        }
                    }
                sp_fc_ok = true;
            }
            o_spv = b.add(nullptr, (size_t)4 * 32 * 3 * sp_nbp * 16);
            o_spc = b.add(nullptr, (size_t)4 * 32 * 3 * sp_nbp);        // ints stored in the float builder (same width)
            for (size_t q = 0; q < (size_t)4 * 32 * 3 * sp_nbp * 16; ++q) b.host[o_spv + q] = 0.f;
            int *ci = reinterpret_cast<int *>(b.host.data() + o_spc);
            for (size_t q = 0; q < (size_t)4 * 32 * 3 * sp_nbp; ++q) ci[q] = 0;
            for (int m = 0; m < 4; ++m)
                for (int wg = 0; wg < 32; ++wg)
                    for (int g = 0; g < 3; ++g) {
                        const size_t br = ((size_t)m * 32 + wg) * 3 + g;
                        const std::vector<int> &cv = cols[br];
                        const float *base = mats[m] + ((size_t)g * H + 16 * wg) * lds_[m];
                        for (size_t k = 0; k < cv.size(); ++k) {
                            ci[br * sp_nbp + k] = cv[k];
                            for (int r = 0; r < 16; ++r) b.host[o_spv + (br * sp_nbp + k) * 16 + r] = base[(size_t)r * lds_[m] + cv[k]];
                        }
                    }
        }
    }
    b.add(nullptr, 64);   // tail padding so vector loads past the last array stay inside the allocation

    wrnn_pack *p = new wrnn_pack();
    p->device = device; p->tr.n_cus = cus; p->tr.C = C; p->tr.mode = w->mode;
    p->dev_bytes = b.host.size() * sizeof(float);
    // W of SURVEY.md section 8(d): every loop parameter the reference touches per step
    p->weight_bytes = sizeof(float) * ((size_t)H * KI + H + 2 * ((size_t)3 * H * H) + (size_t)3 * H * K2 + (size_t)3 * H * H +
                                       4 * 3 * H + 2 * ((size_t)H * K2 + H) + (size_t)C * H + C);
    hipError_t e = hipMalloc((void **)&p->dev, p->dev_bytes);
    if (e != hipSuccess) { set_err("hipMalloc(%zu) failed: %s", p->dev_bytes, hipGetErrorString(e)); delete p; return WRNN_ERR_HIP; }
    e = hipMemcpy(p->dev, b.host.data(), p->dev_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_err("hipMemcpy failed: %s", hipGetErrorString(e)); (void)hipFree(p->dev); delete p; return WRNN_ERR_HIP; }
    const float *base = (const float *)p->dev;
    p->I_w0 = base + o_I_w0; p->I_b = base + o_I_b; p->I_cT = base + o_I_cT;
    p->w_ih1 = base + o_w_ih1; p->w_hh1 = base + o_w_hh1; p->b_ih1 = base + o_b_ih1; p->b_hh1 = base + o_b_hh1;
    p->w_ih2 = base + o_w_ih2; p->w_hh2 = base + o_w_hh2; p->b_ih2 = base + o_b_ih2; p->b_hh2 = base + o_b_hh2;
    p->fc1_w = base + o_fc1_w; p->fc1_b = base + o_fc1_b; p->fc2_w = base + o_fc2_w; p->fc2_b = base + o_fc2_b;
    p->fc3_w = base + o_fc3_w; p->fc3_b = base + o_fc3_b;
    p->w_ih1T = base + o_w_ih1T; p->w_hh1T = base + o_w_hh1T; p->w_ih2T = base + o_w_ih2T; p->w_hh2T = base + o_w_hh2T;
    p->fc1T = base + o_fc1T; p->fc2T = base + o_fc2T; p->fc3T = base + o_fc3T;
    p->c2_wT = base + o_c2_wT; p->c3_wT = base + o_c3_wT; p->c4_wT = base + o_c4_wT;
    p->fc3f = w->mode == WRNN_MODE_MOL ? base + o_fc3f : nullptr;
    p->u1 = base + o_u1;
    p->tr.sp_nbp = sp_nbp; p->tr.sp_max_blocks = sp_max;
    p->sp_vals = sp_nbp ? base + o_spv : nullptr;
    p->sp_cols = sp_nbp ? reinterpret_cast<const int *>(base + o_spc) : nullptr;
    p->sp_fc_max_blocks = sp_fc_max;
    p->sp_fc_vals = sp_fc_ok ? base + o_sfv : nullptr;
    p->sp_fc_cols = sp_fc_ok ? reinterpret_cast<const int *>(base + o_sfc) : nullptr;
    p->tr.struct_bytes = (int32_t)sizeof p->tr; p->tr.sp_fc = sp_fc_ok ? 1 : 0;
    *out = p;
    return WRNN_OK;
}

extern "C" void wrnn_pack_destroy(wrnn_pack *p)
{
    if (!p) return;
    (void)hipFree(p->dev);
    delete p;
}

extern "C" size_t wrnn_pack_weight_bytes(const wrnn_pack *p) { return p ? p->weight_bytes : 0; }

// (a generic pack never runs on wrnn_sparse_kernel; its sp_nbp speaks of the tile-sparse view)
extern "C" int wrnn_pack_sparse_blocks(const wrnn_pack *p) { return p ? (p->tr.sp_nbp && !p->tr.generic ? p->tr.sp_max_blocks : -p->tr.sp_max_blocks) : 0; }
extern "C" int wrnn_pack_sparse_fc_blocks(const wrnn_pack *p) { return p ? (p->sp_fc_vals ? p->sp_fc_max_blocks : -p->sp_fc_max_blocks) : 0; }

extern "C" int wrnn_pack_tile_sparse(const wrnn_pack *p, int32_t kept[6], int32_t total[6])
{
    if (!p) return 0;
    for (int m = 0; m < 6; ++m) {
        if (kept) kept[m] = p->tr.generic ? p->ts_kept[m] : 0;
        if (total) total[m] = p->tr.generic ? p->ts_total[m] : 0;
    }
    return p->tr.generic ? p->ts_view : 0;
}

extern "C" size_t wrnn_pack_tile_bf16(const wrnn_pack *p) { return p && p->tr.generic ? p->bf_bytes : 0; }

struct wrnn_timer {
    int device;
    std::vector<hipEvent_t> ev;     // pairs (start, stop), grown on demand and reused
    int used;                       // events recorded by the last call
};

extern "C" int wrnn_timer_create(int device, wrnn_timer **out)
{
    if (!out) { set_err("NULL argument"); return WRNN_ERR_ARG; }
    const int cus = wrnn_device_cus(device);
    if (cus < 0) return cus;
    wrnn_timer *t = new wrnn_timer();
    t->device = device;
    t->used = 0;
    *out = t;
    return WRNN_OK;
}

extern "C" void wrnn_timer_destroy(wrnn_timer *t)
{
    if (!t) return;
    for (hipEvent_t e : t->ev) (void)hipEventDestroy(e);
    delete t;
}

extern "C" int wrnn_timer_launches(const wrnn_timer *t) { return t ? t->used / 2 : 0; }

extern "C" float wrnn_timer_ms(wrnn_timer *t)
{
    if (!t || t->used < 2) return -1.f;
    float total = 0.f;
    for (int i = 0; i + 1 < t->used; i += 2) {
        if (hipEventSynchronize(t->ev[i + 1]) != hipSuccess) return -1.f;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]) != hipSuccess) return -1.f;
        total += ms;
    }
    return total;
}

namespace {
int timer_mark(wrnn_timer *t, hipStream_t stream)
{
    if (!t) return WRNN_OK;
    if (t->used == (int)t->ev.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        t->ev.push_back(e);
    }
    HIPCHK(hipEventRecord(t->ev[t->used], stream));
    t->used += 1;
    return WRNN_OK;
}

// progress read-out (wrnn_options.progress): a host function enqueued behind the launches of a slab
struct ProgressCtx {
    void (*fn)(int32_t, int32_t, int32_t, void *);
    void *user;
    int32_t done, T, n;
};
void progress_trampoline(void *p)
{
    ProgressCtx *c = static_cast<ProgressCtx *>(p);
    c->fn(c->done, c->T, c->n, c->user);
    delete c;
}
int enqueue_progress(const wrnn_options *o, int done, int T, int n, hipStream_t stream)
{
    if (!o->progress) return WRNN_OK;
    ProgressCtx *c = new ProgressCtx{o->progress, o->progress_user, done, T, n};
    hipError_t e = hipLaunchHostFunc(stream, progress_trampoline, c);
    if (e != hipSuccess) {
        delete c;
        set_err("hipLaunchHostFunc failed: %s", hipGetErrorString(e));
        return WRNN_ERR_HIP;
    }
    return WRNN_OK;
}

enum Kind { K_STREAM, K_GENERIC, K_LOOP, K_DUO, K_OCTO, K_CHAIN, K_SPARSE, K_TILE, K_TILE_SPARSE, K_TILE_BF16, K_TILE_WIDE, N_KINDS };
constexpr int DUO_TAB_FPS = 8;       // rows per segment of the per-slab aux tables: a slab covers at most (DUO_TAB_FPS - 2) hops + 1 steps
constexpr bool DUO_AUTO = true;      // `auto` runs MoL on wrnn_duo_kernel at every depth (round 4, profiles/r04a_probe_new.json: 13.5 vs 16.6 us per step
                                     // with one group in flight, 17.9 vs 21.7 with two, 26.2 vs 36 with four; round 3's kernel paid off from depth 3 on)
constexpr int CHAIN_AUTO_GROUPS = 8;   // `auto` runs calls of up to this many groups (128 segments) on wrnn_chain_kernel: one / two groups per cluster, 10.4 / 13.8 us (RAW: 12.8 / 16.3)
                                       // per step against wrnn_duo_kernel's 12.2 / 16.9; from three groups on the duo kernel wins (profiles/r05i_probe_chain_depths.json)
constexpr bool OCTO_AUTO = false;    // `auto` runs dense MoL batches beyond wrnn_chain_kernel's range on wrnn_octo_kernel (round 6)

// Everything the host knows of a kernel, once: what make_plan, ws_layout, wrnn_plan_segments and wrnn_generate_segments look up by Kind.
struct KindDesc {
    const char *name;
    int units_per_wg;                   // as wrnn_run_info reports it
    int kind_tag;                       // LoopArgs.kind_tag: status word 8, which a continued call must find again
    bool persistent;                    // state and exchange buffer live in the workspace between launches: split into clusters x depth x rounds, slabs of steps,
                                        // and the only kernels that accept a partial step range
    bool slabbed;                       // ... and forms its conditioning in the loop, from per-segment aux tables refilled for every slab
    bool mel_stage;                     // ... and can form the last up-sampling stage too (wrnn_options.mel_stage)
    int (*clusters)(int n_cus);         // 0: the device cannot host it
    int (*max_depth)(int mode);
    size_t (*state_floats)(int G);      // per round
    size_t (*xbuf_bytes)(int G);        // exchange buffer: what the workspace holds ...
    size_t (*xbuf_fill)(int G);         // ... and the prefix a launch at depth G touches (set to the sentinel before it)
    hipError_t (*launch)(const LoopArgs &a, int ncl, int nbp, int mode, hipStream_t s);
};
size_t loop_xbuf_bytes(int) { return XBUF_FLOATS * sizeof(float); }
const KindDesc KINDS[N_KINDS] = {
    /* K_STREAM  */ {"wrnn_stream_kernel", 0, 0, false, false, false},
    /* K_GENERIC */ {"wrnn_generic_kernel", 16, 0, false, false, false},
    /* K_LOOP    */ {"wrnn_loop_kernel", 16, 1, true, false, false, clusters_of_64, loop_max_depth, loop_state_floats, loop_xbuf_bytes, loop_xbuf_bytes,
                     [](const LoopArgs &a, int ncl, int, int mode, hipStream_t s) { return launch_loop(a, ncl, mode, s); }},
    // (wrnn_duo_kernel's launches may differ in depth: the workspace holds all 8 x 4 regions)
    /* K_DUO     */ {"wrnn_duo_kernel", 16, 2, true, true, true, clusters_of_64, [](int) { return duo_max_depth(); }, loop_state_floats,
                     [](int) { return duo_xbuf_bytes_max(); }, duo_xbuf_bytes,
                     [](const LoopArgs &a, int ncl, int, int mode, hipStream_t s) { return launch_duo(a, ncl, mode, s); }},
    // (one 512-thread workgroup per CU, matrix + service waves; MOL: the duo kernel's split, workspace, exchange buffer and state layout, to the depth its LDS carve holds)
    /* K_OCTO    */ {"wrnn_octo_kernel", 16, 5, true, true, true, clusters_of_64, [](int) { return octo_max_depth(); }, loop_state_floats,
                     [](int) { return duo_xbuf_bytes_max(); }, duo_xbuf_bytes,
                     [](const LoopArgs &a, int ncl, int, int mode, hipStream_t s) { return launch_octo(a, ncl, mode, s); }},
    /* K_CHAIN   */ {"wrnn_chain_kernel", 16, 4, true, true, true, chain_clusters, [](int) { return chain_max_depth(); }, chain_state_floats,
                     chain_xbuf_bytes, chain_xbuf_bytes,
                     [](const LoopArgs &a, int, int, int mode, hipStream_t s) { return launch_chain(a, mode, s); }},
    // (16 clusters of 16 CUs, one group each: max_depth is what wrnn_options.depth and `auto` can reach; wrnn_options.sparse_groups = 2 plans two, make_plan)
    /* K_SPARSE  */ {"wrnn_sparse_kernel", 64, 3, true, true, true, sparse_clusters, [](int) { return 1; }, sparse_state_floats,
                     sparse_xbuf_bytes, sparse_xbuf_bytes,
                     [](const LoopArgs &a, int, int nbp, int mode, hipStream_t s) { return launch_sparse(a, nbp, mode, s); }},
    // (wrnn_generic_kernel's dataflow and pack, one workgroup per 16 segments; on request)
    /* K_TILE    */ {"wrnn_tile_kernel", 16, 0, false, false, false},
    // (wrnn_tile_kernel with the GRU -- and fc1 / fc2 -- stages on the pack's tile-sparse view; on request)
    /* K_TILE_SPARSE */ {"wrnn_tile_sparse_kernel", 16, 0, false, false, false},
    // (wrnn_tile_kernel with the eight matrices in bfloat16, on the bf16 MFMA; on request)
    /* K_TILE_BF16 */ {"wrnn_tile_bf16_kernel", 16, 0, false, false, false},
    // (wrnn_tile_kernel with the rows of every stage spread over wrnn_options.clusters = 2, 4 or 8 workgroups per tile; on request)
    /* K_TILE_WIDE */ {"wrnn_tile_wide_kernel", 16, 0, false, false, false},
};

// what a call will run: kernel, split, rounds, slab length
struct Plan {
    Kind kind;
    int ncl, G, rounds, per_round, slab, ngr_max;
    int tab_fps;                        // slabbed kernels: rows per segment of the per-slab aux tables
    int t0, t1;
};

struct WsLayout {
    size_t status, xcc, segs, melc, c2f, c3f, c4f;
    size_t cI, npre;                    // stream kernel: whole-T conditioning; persistent kernels: one slab of derived MOL noise
    size_t nlib;                        // wrnn_options.noise_lib: the noise the library draws, in the layout of `noise` -- one slab (persistent kernels) or all T steps
    size_t xbuf, state, cIf;            // loop kernel: exchange buffer, per-round state, conditioning slab
    size_t wide;                        // wrnn_tile_wide_kernel: flag block | per-(tile, stage) hand-off buffers
    size_t total;
};
size_t al(size_t x) { return (x + 255) / 256 * 256; }

// a caller's struct, of this or another version of the header: its first struct_bytes bytes, the rest zero (NULL: all defaults)
template <class S> S norm_struct(const S *in)
{
    S s;
    memset(&s, 0, sizeof s);
    if (in) memcpy(&s, in, in->struct_bytes > 0 && (size_t)in->struct_bytes < sizeof s ? (size_t)in->struct_bytes : sizeof s);
    s.struct_bytes = (int32_t)sizeof s;
    return s;
}
// ... and planned as the WHOLE call: the workspace and the split of a partial-range call are the whole call's
wrnn_options whole_call(const wrnn_options *opt)
{
    wrnn_options o = norm_struct(opt);
    o.t_begin = 0; o.t_end = 0;
    return o;
}

// B segments = groups of <= SEG on ncl clusters x G slots: the requested depth, or as deep as the segments fill evenly -- rounds =
// ceil(groups / (ncl * gmax)), then the shallowest depth that still needs only that many rounds (deeper pipelines hide the exchange
// latency; empty slots cost nothing) --, then balanced rounds of whole segments, every round cut into <= ncl * G groups
void plan_split(Plan *pl, int B, int ncl, int gmax, int depth)
{
    const int groups = (B + SEG - 1) / SEG;
    int g = depth;
    if (g < 1 || g > gmax) {
        const int rounds = (groups + ncl * gmax - 1) / (ncl * gmax);
        g = (groups + ncl * rounds - 1) / (ncl * rounds);
        if (g < 1) g = 1;
        if (g > gmax) g = gmax;
    }
    pl->ncl = ncl; pl->G = g;
    pl->rounds = (groups + ncl * g - 1) / (ncl * g);
    pl->per_round = (B + pl->rounds - 1) / pl->rounds;
    pl->ngr_max = (pl->per_round + SEG - 1) / SEG;
    if (pl->ngr_max > ncl * g) { pl->rounds += 1; pl->per_round = (B + pl->rounds - 1) / pl->rounds; pl->ngr_max = (pl->per_round + SEG - 1) / SEG; }
}

// steps per slab when the caller names none = what a slab holds: wrnn_loop_kernel -- the hoisted conditioning cI (2 KB per segment-step) + the
// derived MoL noise; the slabbed kernels form cI in the loop: only the derived noise (44 B per segment-step)
// wrnn_options.noise_lib, RAW on a slabbed kernel: the slab also holds its noise (C floats per segment-step) -- as much as fits NOISE_LIB_SLAB_BYTES
constexpr size_t NOISE_LIB_SLAB_BYTES = (size_t)2 << 30;      // (the slice of noise WaveRNN.generate keeps resident when the caller draws it: noise_chunk_bytes)
int default_slab(const Plan &pl, int mode, int C, bool noise_lib)
{
    const int most = KINDS[pl.kind].slabbed ? 4096 : 1024;
    int slab = most;
    if (!KINDS[pl.kind].slabbed) slab = (int)((96u << 20) / ((size_t)pl.ngr_max * SEG * H * sizeof(float)));
    else if (mode == WRNN_MODE_MOL) slab = (int)((32u << 20) / ((size_t)pl.per_round * 11 * sizeof(float) * pl.rounds));
    else if (noise_lib) {
        const size_t fit = NOISE_LIB_SLAB_BYTES / ((size_t)pl.per_round * pl.rounds * C * sizeof(float));
        slab = fit < (size_t)most ? (int)fit : most;
    }
    return slab < 16 ? 16 : slab > most ? most : slab;
}

// Which kernel a call runs on, and how it is cut.  algo = a kernel by name: that kernel, or an error that says what it needs (WRNN_ERR_ARG: this
// pack never runs on it; WRNN_ERR_RESIDENCY: this device is too small).  `auto`, shipped dims, MOL or RAW with 512 classes:
//   a MOL pack whose GRU matrices are block-sparse (sp_nbp), >= 256 CUs                      wrnn_sparse_kernel (a sparse RAW pack: on request only)
//   else up to CHAIN_AUTO_GROUPS groups (128 segments), >= 256 CUs                           wrnn_chain_kernel
//   else >= 256 CUs                                                                          wrnn_duo_kernel, always on 4 clusters
//   else >= 64 CUs                                                                           wrnn_loop_kernel on 1 or 2 clusters, no more than there are groups
//   else, and RAW with fewer classes                                                         wrnn_stream_kernel
// non-shipped dims, and the shipped ones with more than 512 RAW classes (a generic pack): wrnn_generic_kernel. wrnn_duo_kernel on 1 or 2 clusters (>= 64 CUs) and wrnn_octo_kernel (MOL, >= 256 CUs) run on request only.
// wrnn_options.depth is honoured up to the kernel's max_depth; .clusters (1, 2, 4) only where loop / duo / octo is planned (`auto` on fewer than 4
// clusters: wrnn_loop_kernel).
int make_plan(const wrnn_plan_traits *p, int B, int T, const wrnn_options *o, Plan *pl)
{
    const bool shape_ok = (p->mode == WRNN_MODE_MOL) || (p->C == H);
    pl->t0 = o->t_begin; pl->t1 = o->t_end;
    if (pl->t0 == 0 && pl->t1 == 0) pl->t1 = T;
    if (pl->t0 < 0 || pl->t1 > T || pl->t0 >= pl->t1) { set_err("bad step range [%d, %d) of T=%d", pl->t0, pl->t1, T); return WRNN_ERR_ARG; }
    const bool partial = pl->t0 != 0 || pl->t1 != T;
    const int algo = o->algo;
    if (algo != WRNN_ALGO_AUTO && algo != WRNN_ALGO_STREAM && algo != WRNN_ALGO_LOOP && algo != WRNN_ALGO_SPARSE && algo != WRNN_ALGO_DUO && algo != WRNN_ALGO_CHAIN &&
        algo != WRNN_ALGO_OCTO && algo != WRNN_ALGO_TILE && algo != WRNN_ALGO_TILE_SPARSE && algo != WRNN_ALGO_TILE_BF16) {
        set_err("unknown algo %d", algo);
        return WRNN_ERR_ARG;
    }
    if (o->sparse_groups < 0 || o->sparse_groups > sparse_max_slots()) {
        set_err("wrnn_options.sparse_groups = %d: 0 or 1 (one group per cluster) or 2", o->sparse_groups);
        return WRNN_ERR_ARG;
    }
    if (o->noise_lib != 0 && o->noise_lib != 1) {
        set_err("wrnn_options.noise_lib = %d: 0 (the caller's `noise`) or 1 (the library draws it)", o->noise_lib);
        return WRNN_ERR_ARG;
    }
    const bool two_groups = o->sparse_groups == 2;
    const int groups = (B + SEG - 1) / SEG;
    pl->kind = K_STREAM; pl->ncl = 0; pl->G = 0; pl->rounds = 1; pl->per_round = B; pl->slab = T; pl->ngr_max = groups;
    if (algo == WRNN_ALGO_TILE) {       // on request only: wrnn_generic_kernel's dataflow for 16 segments per workgroup (csrc/wrnn_tile.hip)
        // wrnn_options.clusters = 2, 4, 8: the rows of every stage on that many workgroups per tile (csrc/wrnn_tile_wide.hip); 0, 1: wrnn_tile_kernel
        const int width = o->clusters;
        if (width != 0 && width != 1 && width != 2 && width != 4 && width != 8) {
            set_err("wrnn_options.clusters = %d under algo tile: 0 or 1 (wrnn_tile_kernel, one workgroup per tile) or 2, 4, 8 (wrnn_tile_wide_kernel: that many "
                    "workgroups per tile)", width);
            return WRNN_ERR_ARG;
        }
        const bool wide = width > 1;
        const char *const kn = wide ? "wrnn_tile_wide_kernel" : "wrnn_tile_kernel";
        if (!p->generic) {
            set_err("%s runs generic packs only (non-shipped dims, or RAW with more than %d classes): this pack has the shipped dims -- algo auto "
                    "picks its kernel", kn, H);
            return WRNN_ERR_ARG;
        }
        if (!tile_dims_ok(p->gH, p->gF, p->gM, p->gA, p->C, p->mode)) {
            set_err("%s: rnn %d, fc %d, feat %d, aux %d, %d classes need %zu bytes of LDS per workgroup, the limit is %d (and RAW: <= 2048 classes); "
                    "algo auto runs this pack on wrnn_generic_kernel", kn, p->gH, p->gF, p->gM, p->gA, p->C, tile_lds_bytes(p->gH, p->gF, p->gM, p->gA, p->C), 160 * 1024);
            return WRNN_ERR_ARG;
        }
        if (partial) { set_err("a partial step range needs a persistent loop kernel"); return WRNN_ERR_ARG; }
        if (two_groups) { set_err("wrnn_options.sparse_groups = 2: only wrnn_sparse_kernel runs two groups per cluster (this call runs on %s)", kn); return WRNN_ERR_ARG; }
        if (wide && (long)groups * width > p->n_cus) {
            // ONE round, the W members of every tile co-resident: a workgroup holds a CU's LDS
            set_err("wrnn_tile_wide_kernel: %d segments are %d tiles of 16, and %d workgroups per tile need %ld CUs; this device has %d: width %d takes at most %d "
                    "segments here -- plain algo tile (wrnn_options.clusters = 0) runs this call", B, groups, width, (long)groups * width, p->n_cus, width,
                    p->n_cus / width * SEG);
            return WRNN_ERR_ARG;
        }
        pl->kind = wide ? K_TILE_WIDE : K_TILE;
        if (wide) pl->ncl = width;
        return WRNN_OK;
    }
    if (algo == WRNN_ALGO_TILE_SPARSE) {        // on request only: wrnn_tile_kernel on the pack's tile-sparse view (csrc/wrnn_tile_sparse.hip)
        if (!p->generic) {
            set_err("wrnn_tile_sparse_kernel runs generic packs only (non-shipped dims, or RAW with more than %d classes): this pack has the shipped dims -- algo "
                    "auto picks its kernel, wrnn_sparse_kernel for a block-sparse one", H);
            return WRNN_ERR_ARG;
        }
        if (o->clusters > 1) {
            set_err("wrnn_options.clusters = %d under algo tile_sparse: only the float32 tile kernel (algo tile) has the wide form", o->clusters);
            return WRNN_ERR_ARG;
        }
        if (p->sp_nbp <= 0) {
            static const char *const names[4] = {"rnn1.weight_ih", "rnn1.weight_hh", "rnn2.weight_ih", "rnn2.weight_hh"};
            const int v = -p->sp_nbp - 1;
            if (p->gH % 16) set_err("wrnn_tile_sparse_kernel: this pack has no tile-sparse view -- rnn %d is no multiple of 16 (a block row is 16 rows of one gate); "
                                    "algo tile runs it dense", p->gH);
            else if (p->sp_nbp < 0 && v / 1001 < 4)
                set_err("wrnn_tile_sparse_kernel: this pack has no tile-sparse view -- %.1f %% of the 16x1 blocks of %s survive, a view needs at most 41 %% in each of "
                        "the four GRU matrices; algo tile runs it dense", 0.1 * (v % 1001), names[v / 1001]);
            else set_err("wrnn_tile_sparse_kernel: this pack has no tile-sparse view (wrnn_pack_tile_sparse() == 0); algo tile runs it dense");
            return WRNN_ERR_ARG;
        }
        if (!tile_dims_ok(p->gH, p->gF, p->gM, p->gA, p->C, p->mode)) {
            set_err("wrnn_tile_sparse_kernel: rnn %d, fc %d, feat %d, aux %d, %d classes need %zu bytes of LDS per workgroup, the limit is %d (and RAW: <= 2048 classes); "
                    "algo auto runs this pack on wrnn_generic_kernel", p->gH, p->gF, p->gM, p->gA, p->C, tile_lds_bytes(p->gH, p->gF, p->gM, p->gA, p->C), 160 * 1024);
            return WRNN_ERR_ARG;
        }
        if (partial) { set_err("a partial step range needs a persistent loop kernel"); return WRNN_ERR_ARG; }
        if (two_groups) { set_err("wrnn_options.sparse_groups = 2: only wrnn_sparse_kernel runs two groups per cluster (this call runs on wrnn_tile_sparse_kernel)"); return WRNN_ERR_ARG; }
        pl->kind = K_TILE_SPARSE;
        return WRNN_OK;
    }
    if (algo == WRNN_ALGO_TILE_BF16) {          // on request only: wrnn_tile_kernel on the pack's bf16 view (csrc/wrnn_tile_bf16.hip)
        if (!p->generic) {
            set_err("wrnn_tile_bf16_kernel runs generic packs only (non-shipped dims, or RAW with more than %d classes): this pack has the shipped dims -- algo auto "
                    "picks its kernel", H);
            return WRNN_ERR_ARG;
        }
        if (o->clusters > 1) {
            set_err("wrnn_options.clusters = %d under algo tile_bf16: only the float32 tile kernel (algo tile) has the wide form", o->clusters);
            return WRNN_ERR_ARG;
        }
        if (!tile_dims_ok(p->gH, p->gF, p->gM, p->gA, p->C, p->mode)) {
            set_err("wrnn_tile_bf16_kernel: rnn %d, fc %d, feat %d, aux %d, %d classes need %zu bytes of LDS per workgroup, the limit is %d (and RAW: <= 2048 classes); "
                    "algo auto runs this pack on wrnn_generic_kernel", p->gH, p->gF, p->gM, p->gA, p->C, tile_lds_bytes(p->gH, p->gF, p->gM, p->gA, p->C), 160 * 1024);
            return WRNN_ERR_ARG;
        }
        if (p->sp_fc & 2) {
            set_err("wrnn_tile_bf16_kernel: this pack has no bf16 view (wrnn_pack_tile_bf16() == 0) -- one of its weights is not finite or rounds to +-inf in "
                    "bfloat16; algo tile runs it in float32");
            return WRNN_ERR_ARG;
        }
        if (partial) { set_err("a partial step range needs a persistent loop kernel"); return WRNN_ERR_ARG; }
        if (two_groups) { set_err("wrnn_options.sparse_groups = 2: only wrnn_sparse_kernel runs two groups per cluster (this call runs on wrnn_tile_bf16_kernel)"); return WRNN_ERR_ARG; }
        pl->kind = K_TILE_BF16;
        return WRNN_OK;
    }
    if (p->generic) {           // non-shipped hparams: the dimension-generic kernel is the only one that takes them without being asked for by name
        if (algo != WRNN_ALGO_AUTO && algo != WRNN_ALGO_STREAM) {
            set_err("this pack has non-shipped dims (rnn %d, fc %d, feat %d, aux %d): only the generic kernel (algo auto / stream) runs it", p->gH, p->gF, p->gM, p->gA);
            return WRNN_ERR_ARG;
        }
        if (partial) { set_err("a partial step range needs a persistent loop kernel"); return WRNN_ERR_ARG; }
        if (two_groups) { set_err("wrnn_options.sparse_groups = 2: only wrnn_sparse_kernel runs two groups per cluster (this call runs on wrnn_generic_kernel)"); return WRNN_ERR_ARG; }
        pl->kind = K_GENERIC;
        return WRNN_OK;
    }
    // ---- what was asked for by name must be possible
    const int ccl = KINDS[K_CHAIN].clusters(p->n_cus), scl = KINDS[K_SPARSE].clusters(p->n_cus), lcl = KINDS[K_LOOP].clusters(p->n_cus);
    const bool chain_hw = shape_ok && ccl >= 1;
    if (algo == WRNN_ALGO_CHAIN && !chain_hw) {
        set_err("wrnn_chain_kernel needs MOL or RAW with 512 classes, and >= 256 CUs (C = %d, device: %d CUs)", p->C, p->n_cus);
        return !shape_ok ? WRNN_ERR_ARG : WRNN_ERR_RESIDENCY;
    }
    if (algo == WRNN_ALGO_SPARSE && (!p->sp_nbp || scl < 1)) {
        set_err("block-sparse kernel needs MOL or RAW with 512 classes, >= 256 CUs and GRU matrices with <= 64 surviving 16x1 blocks per block row "
                "(this pack: mode %s, %d classes, up to %d blocks; device: %d CUs)", p->mode == WRNN_MODE_MOL ? "MOL" : "RAW", p->C, p->sp_max_blocks, p->n_cus);
        return (!p->sp_nbp) ? WRNN_ERR_ARG : WRNN_ERR_RESIDENCY;
    }
    if (algo == WRNN_ALGO_OCTO && (p->mode != WRNN_MODE_MOL || KINDS[K_OCTO].clusters(p->n_cus) != MAXCL)) {
        set_err("wrnn_octo_kernel needs MOL and >= 256 CUs (mode %d, device has %d CUs)", p->mode, p->n_cus);
        return p->mode != WRNN_MODE_MOL ? WRNN_ERR_ARG : WRNN_ERR_RESIDENCY;
    }
    if (algo == WRNN_ALGO_DUO && (!shape_ok || KINDS[K_DUO].clusters(p->n_cus) < 1)) {
        set_err("the two-workgroups-per-CU loop kernel needs MOL or RAW with 512 classes, and >= 64 CUs (C = %d, device has %d CUs)", p->C, p->n_cus);
        return !shape_ok ? WRNN_ERR_ARG : WRNN_ERR_RESIDENCY;
    }
    if (algo == WRNN_ALGO_LOOP && !(shape_ok && lcl >= 1)) {     // (RESIDENCY for the shape too: as it has always answered)
        set_err("the loop kernel needs >= 64 CUs and (MOL or RAW with 512 classes); device has %d CUs, C=%d", p->n_cus, p->C);
        return WRNN_ERR_RESIDENCY;
    }
    // ---- the kernel and its clusters
    const bool sparse_auto = p->sp_nbp && p->mode == WRNN_MODE_MOL;      // (RAW: the sparse kernel's summation order is not the oracle's -- `auto` keeps the dense kernels)
    Kind kind = K_STREAM;
    int ncl = 0;
    if (algo == WRNN_ALGO_CHAIN || (algo == WRNN_ALGO_AUTO && chain_hw && groups <= CHAIN_AUTO_GROUPS && !sparse_auto)) {
        // one workgroup per CU, one instruction stream per wave.  `auto`: <= 64 segments (one utterance of BASELINE config 2 / 3): one group per 64-CU
        // cluster, a step is the latency of one chain; <= 128: two groups per cluster
        kind = K_CHAIN; ncl = ccl;
    } else if (algo == WRNN_ALGO_SPARSE || (algo == WRNN_ALGO_AUTO && sparse_auto && scl >= 1)) {
        // (round 5) one group of 16 segments per cluster: the step is the latency of one chain, and sixteen chains run side by side
        kind = K_SPARSE; ncl = scl;
    } else if (algo != WRNN_ALGO_STREAM && shape_ok && lcl >= 1) {
        ncl = lcl;
        if (o->clusters == 1 || o->clusters == 2 || o->clusters == 4) ncl = o->clusters < ncl ? o->clusters : ncl;
        else if (groups < ncl && !(DUO_AUTO && algo != WRNN_ALGO_LOOP && ncl == MAXCL)) {
            // no more clusters than groups (rounded up to 1, 2, 4).  Not for the duo kernel: its grid is always 4 clusters (a cluster
            // without a group leaves at once), so that a small batch sits on whole XCDs exactly as a large one does
            int c2 = 1; while (c2 < groups) c2 *= 2; if (c2 < ncl) ncl = c2;
        }
        // the two-workgroups-per-CU form: on request, or when `auto` has all four clusters (busy time bounds a step there)
        kind = K_LOOP;
        if (algo == WRNN_ALGO_DUO || (algo == WRNN_ALGO_AUTO && DUO_AUTO && ncl == MAXCL)) kind = K_DUO;
        if (algo == WRNN_ALGO_OCTO || (kind == K_DUO && algo == WRNN_ALGO_AUTO && OCTO_AUTO && p->mode == WRNN_MODE_MOL && !o->clusters)) kind = K_OCTO;
    }
    const KindDesc &k = KINDS[kind];
    pl->kind = kind;
    // two groups per cluster of wrnn_sparse_kernel: on request only, and only what is instantiated -- MOL with gathered fc stages (the dense fc tiles leave
    // no register room: <64, false> spills as it is), no phase clocks
    if (two_groups) {
        if (kind != K_SPARSE) {
            set_err("wrnn_options.sparse_groups = 2: only wrnn_sparse_kernel runs two groups per cluster (this call runs on %s)", k.name);
            return WRNN_ERR_ARG;
        }
        if (p->mode != WRNN_MODE_MOL) { set_err("wrnn_options.sparse_groups = 2: wrnn_sparse_kernel's 9-bit RAW form is built with one group per cluster only"); return WRNN_ERR_ARG; }
        if (!p->sp_fc || (o->tuning & 2048)) {
            set_err("wrnn_options.sparse_groups = 2: needs a pack whose Linear layers are block-sparse too (wrnn_pack_sparse_fc_blocks() > 0) and their gathered fc "
                    "stages: the dense fc tiles leave no registers for a second group");
            return WRNN_ERR_ARG;
        }
        if (o->phase_clocks && !(o->tuning & 64)) { set_err("wrnn_options.sparse_groups = 2: the phase-clock build of wrnn_sparse_kernel has one group per cluster only"); return WRNN_ERR_ARG; }
    }
    if (k.persistent) {
        if (two_groups) plan_split(pl, B, ncl, sparse_max_slots(), sparse_max_slots());      // depth 2, rounds = ceil(groups / 32)
        else plan_split(pl, B, ncl, k.max_depth(p->mode), o->depth);
        pl->slab = o->slab_steps >= 1 ? o->slab_steps : default_slab(*pl, p->mode, p->C, o->noise_lib != 0);      // (an explicit slab length is taken as given -- short slabs included: tests)
        if (pl->slab > T) pl->slab = T;
        pl->tab_fps = DUO_TAB_FPS;
    } else if (partial) {
        set_err("a partial step range [%d, %d) needs a persistent loop kernel", pl->t0, pl->t1);
        return WRNN_ERR_ARG;
    }
    // the kernels that form their conditioning in the loop index the per-segment, per-slab aux tables with 32-bit byte offsets inside one buffer
    // resource: refused HERE, so that wrnn_plan_segments / wrnn_workspace_bytes_segments report it and nothing has been queued when a call fails
    if (k.slabbed && ((size_t)B * pl->tab_fps + 1) * 3 * H * sizeof(float) >= 0x7FFFF000ull) {
        set_err("%d segments in one call: the per-slab aux tables exceed a 2 GB buffer resource; split the call (generate_corpus caps a launch at 4096 segments)", B);
        return WRNN_ERR_ARG;
    }
    return WRNN_OK;
}

// noise_lib: the call draws its own noise (wrnn_options.noise_lib) -- appended, so that every other offset is what it is without
WsLayout ws_layout(const wrnn_plan_traits *p, const Plan &pl, int B, int T, int n_frames, bool noise_lib)
{
    const size_t noise_row = (size_t)B * (p->mode == WRNN_MODE_MOL ? 11 : p->C) * sizeof(float);      // one step of `noise`
    const KindDesc &k = KINDS[pl.kind];
    WsLayout l;
    memset(&l, 0, sizeof l);
    size_t o = 0;
    l.status = o; o = al(o + STATUS_WORDS * sizeof(unsigned));
    l.xcc = o;    o = al(o + XCC_WORDS * sizeof(unsigned));
    l.segs = o;   o = al(o + (size_t)3 * B * sizeof(int));       // positions | limits | mel offsets (wrnn_options.mel_stage)
    l.melc = o;   o = al(o + (size_t)3 * LAST_SCALE * sizeof(float));
    if (pl.kind == K_GENERIC || pl.kind == K_TILE || pl.kind == K_TILE_SPARSE || pl.kind == K_TILE_BF16 || pl.kind == K_TILE_WIDE) {
        l.nlib = o; if (noise_lib) o = al(o + (size_t)T * noise_row);
        l.wide = o;         // (behind everything wrnn_tile_kernel's workspace holds; by the tile count and the dims, not by T)
        if (pl.kind == K_TILE_WIDE) o = al(o + tile_wide_flag_bytes(pl.ngr_max) + tile_wide_xbuf_bytes(pl.ngr_max, p->gH, p->gF, p->C, p->mode));
        l.total = o;
        return l;
    }
    // per-frame aux tables: one row per frame of the call's conditioning (+ the zero row) -- or, for a slabbed kernel, per SEGMENT and
    // slab: (slab - 1) / hop + 2 rows per segment (+ the zero row), refilled for every slab: independent of the corpus' length
    const size_t tab_rows = k.slabbed ? (size_t)B * pl.tab_fps + 1 : (size_t)n_frames + 1;
    l.c2f = o;    o = al(o + tab_rows * 3 * H * sizeof(float));
    l.c3f = o;    o = al(o + tab_rows * H * sizeof(float));
    l.c4f = o;    o = al(o + tab_rows * H * sizeof(float));
    if (k.persistent) {
        l.xbuf = o;  o = al(o + k.xbuf_bytes(pl.G));
        l.state = o; o = al(o + (size_t)pl.rounds * k.state_floats(pl.G) * sizeof(float));
        l.cIf = o;   if (!k.slabbed) o = al(o + (size_t)pl.slab * pl.ngr_max * SEG * H * sizeof(float));      // (a slabbed kernel forms cI in the loop)
        l.npre = o;  if (p->mode == WRNN_MODE_MOL) o = al(o + (size_t)pl.slab * 11 * B * sizeof(float));      // derived MOL noise of one slab
    } else {
        l.cI = o;    o = al(o + (size_t)T * B * H * sizeof(float));
        l.npre = o;
    }
    l.nlib = o;   if (noise_lib) o = al(o + (size_t)(k.persistent ? pl.slab : T) * noise_row);
    l.total = o;
    return l;
}
// p / hop == __umulhi(p, magic) >> shift for every 0 <= p < 2^31 (Granlund-Montgomery, N = 31: magic = ceil(2^(31 + s) / hop) with
// s = ceil(log2 hop) fits 32 bits and its error term is <= 2^s); checked below on the multiples of hop and their neighbours.  magic = 0:
// the kernel divides.
void hop_magic(int hop, unsigned *magic, int *shift)
{
    *magic = 0u; *shift = 0;
    if (hop < 2) return;
    int s = 0;
    while ((1ll << s) < hop) ++s;
    const unsigned long long m = ((1ull << (31 + s)) + (unsigned long long)hop - 1ull) / (unsigned long long)hop;
    if (m >> 32) return;
    const int sh = s - 1;
    for (long long q = 0; q * hop < (1ll << 31); q += 997) {            // spot check (the bound is a theorem; this guards the arithmetic)
        for (long long p = q * hop - 1; p <= q * hop + 1; ++p) {
            if (p < 0 || p >= (1ll << 31)) continue;
            if ((long long)(((unsigned long long)p * m) >> (32 + sh)) != p / hop) return;
        }
    }
    *magic = (unsigned)m; *shift = sh;
}

int check_geometry(const wrnn_geometry *g)
{
    if (!g) { set_err("NULL geometry"); return WRNN_ERR_ARG; }
    if (g->B < 1 || g->T < 1 || g->L < 1 || g->hop < 1 || g->n_frames < 1 || g->stride < 0) {
        set_err("bad geometry B=%d T=%d stride=%d L=%d hop=%d n_frames=%d", g->B, g->T, g->stride, g->L, g->hop, g->n_frames);
        return WRNN_ERR_ARG;
    }
    if ((long)g->n_frames * g->hop < g->L) { set_err("n_frames*hop < L"); return WRNN_ERR_ARG; }
    if ((double)g->B * g->stride + g->T > 2.0e9) { set_err("geometry overflows int32"); return WRNN_ERR_ARG; }
    return WRNN_OK;
}
int check_segments(int B, int T, const int32_t *seg_pos, const int32_t *seg_lim, int L, int hop, int n_frames)
{
    if (B < 1 || T < 1 || L < 1 || hop < 1 || n_frames < 1 || !seg_pos || !seg_lim) {
        set_err("bad segment table B=%d T=%d L=%d hop=%d n_frames=%d", B, T, L, hop, n_frames);
        return WRNN_ERR_ARG;
    }
    if ((long)n_frames * hop < L) { set_err("n_frames*hop < L"); return WRNN_ERR_ARG; }
    for (int b = 0; b < B; ++b) {
        if (seg_pos[b] < 0 || seg_lim[b] < 0 || seg_lim[b] > L || (double)seg_pos[b] + T > 2.0e9) {
            set_err("segment %d: pos=%d lim=%d outside [0,%d]", b, seg_pos[b], seg_lim[b], L);
            return WRNN_ERR_ARG;
        }
    }
    return WRNN_OK;
}
// what wrnn_plan_segments (`out`) and wrnn_workspace_bytes_segments (`ws_bytes`) answer; either may be NULL
int plan_report(const wrnn_plan_traits *tr, int B, int T, int n_frames, const wrnn_options &o, wrnn_run_info *out, size_t *ws_bytes)
{
    Plan pl;
    const int rc = make_plan(tr, B, T, &o, &pl);
    if (rc != WRNN_OK) return rc;
    if (out) {
        memset(out, 0, sizeof *out);
        out->kernel = KINDS[pl.kind].name; out->units_per_wg = KINDS[pl.kind].units_per_wg;
        out->clusters = pl.ncl; out->depth = pl.G; out->rounds = pl.rounds; out->slab_steps = pl.slab;
    }
    if (ws_bytes) *ws_bytes = ws_layout(tr, pl, B, T, n_frames, o.noise_lib != 0).total;
    return WRNN_OK;
}

// A WATCHED call (wrnn_generate_segments_watched): the one-launch kernels publish how far they have got, one word per workgroup that writes `out`
// (wrnn_generic_kernel: one per segment; the tile kernels: one per tile of 16 segments -- wrnn_tile_wide_kernel: member 0 of the tile).
struct Watch {
    unsigned *progress;
    int words, every;
};
bool watchable(Kind k) { return k == K_GENERIC || k == K_TILE || k == K_TILE_SPARSE || k == K_TILE_BF16 || k == K_TILE_WIDE; }
// what a watched call may be: planned whole onto one of the five kernels.  `words` <- the words it writes.  w: NULL = only that (wrnn_watch_words)
int watch_check(const wrnn_plan_traits *tr, int B, int T, const wrnn_options &o, const Watch *w, bool have_progress, int *words)
{
    wrnn_options whole = o;
    whole.t_begin = 0; whole.t_end = 0;
    Plan pl;
    const int rc = make_plan(tr, B, T, &whole, &pl);
    if (rc != WRNN_OK) return rc;
    const char *const kn = KINDS[pl.kind].name;
    if (!watchable(pl.kind)) {
        set_err("a watched call runs on wrnn_generic_kernel, wrnn_tile_kernel, wrnn_tile_sparse_kernel, wrnn_tile_bf16_kernel or wrnn_tile_wide_kernel, the "
                "kernels that are launched once for all steps: this call plans onto %s -- the resumable kernels stream through wrnn_options.t_begin / t_end "
                "instead", kn);
        return WRNN_ERR_ARG;
    }
    if (o.t_begin != 0 || (o.t_end != 0 && o.t_end != T)) {
        set_err("a watched call runs whole: the step range [%d, %d) of T = %d is partial, and %s (planned) does not continue a call", o.t_begin, o.t_end, T, kn);
        return WRNN_ERR_ARG;
    }
    const int need = pl.kind == K_GENERIC ? B : (B + SEG - 1) / SEG;
    if (words) *words = need;
    if (!w) return WRNN_OK;
    if (!have_progress) { set_err("a watched call needs `progress`: it is NULL (planned: %s, %d words)", kn, need); return WRNN_ERR_ARG; }
    if (w->every < 1) { set_err("progress_every = %d: a watched call publishes every progress_every >= 1 steps (planned: %s)", w->every, kn); return WRNN_ERR_ARG; }
    if (w->words < need) {
        set_err("progress_words = %d: %s publishes one word per workgroup that writes `out`, %d for %d segments (wrnn_watch_words)", w->words, kn, need, B);
        return WRNN_ERR_ARG;
    }
    return WRNN_OK;
}
}  // namespace

extern "C" size_t wrnn_workspace_bytes_segments(const wrnn_pack *p, int32_t n_segments, int32_t T, int32_t n_frames,
                                                const wrnn_options *opt)
{
    if (!p || n_segments < 1 || T < 1 || n_frames < 1) return 0;
    size_t bytes = 0;
    (void)plan_report(&p->tr, n_segments, T, n_frames, whole_call(opt), nullptr, &bytes);
    return bytes;
}

extern "C" int wrnn_plan_segments(const wrnn_pack *p, int32_t n_segments, int32_t T, const wrnn_options *opt, wrnn_run_info *out)
{
    if (!p || !out || n_segments < 1 || T < 1) { set_err("bad argument"); return WRNN_ERR_ARG; }
    return plan_report(&p->tr, n_segments, T, 1, whole_call(opt), out, nullptr);
}

extern "C" size_t wrnn_workspace_bytes(const wrnn_pack *p, const wrnn_geometry *g, const wrnn_options *opt)
{
    if (!p || check_geometry(g) != WRNN_OK) return 0;
    return wrnn_workspace_bytes_segments(p, g->B, g->T, g->n_frames, opt);
}

// the one body of wrnn_generate_segments (watch == NULL) and wrnn_generate_segments_watched
static int generate_segments(const wrnn_pack *p, int32_t B, int32_t T, const int32_t *seg_pos,
                             const int32_t *seg_lim, int32_t L, int32_t hop, int32_t n_frames,
                             const float *mels_up, const float *aux, const float *noise, float *out,
                             void *workspace, size_t workspace_bytes, const wrnn_options *opt, void *stream_, const Watch *watch)
{
    const wrnn_options opts = norm_struct(opt), *o = &opts;
    const bool lib_noise = o->noise_lib == 1;       // (any other value but 0: make_plan refuses it)
    if (lib_noise && noise) {
        set_err("wrnn_options.noise_lib = 1: the library draws the noise itself -- `noise` must be NULL (the tensor passed would not be read)");
        return WRNN_ERR_ARG;
    }
    if (!p || !mels_up || !aux || (!noise && !lib_noise) || !out || !workspace) { set_err("NULL argument"); return WRNN_ERR_ARG; }
    int rc = check_segments(B, T, seg_pos, seg_lim, L, hop, n_frames);
    if (rc != WRNN_OK) return rc;
    int watch_need = 0;     // a watched call: refused here, before anything is queued, unless it is planned whole onto a one-launch kernel
    if (watch && (rc = watch_check(&p->tr, B, T, opts, watch, watch->progress != nullptr, &watch_need)) != WRNN_OK) return rc;
    Plan pl;      // (kernel, split and workspace layout do not depend on the step range: a continuation lands on the whole call's)
    if ((rc = make_plan(&p->tr, B, T, o, &pl)) != WRNN_OK) return rc;
    const KindDesc &k = KINDS[pl.kind];
    const WsLayout l = ws_layout(&p->tr, pl, B, T, n_frames, lib_noise);
    if (workspace_bytes < l.total) { set_err("workspace %zu < required %zu", workspace_bytes, l.total); return WRNN_ERR_WORKSPACE; }
    if (((uintptr_t)workspace & 255) != 0) { set_err("workspace must be 256-byte aligned"); return WRNN_ERR_ARG; }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard dg(p->device);
    HIPCHK(dg.err);
    char *ws = (char *)workspace;
    const bool mol_mode = p->tr.mode == WRNN_MODE_MOL;
    wrnn_timer *timer = o->timer;
    if (timer && pl.t0 == 0) timer->used = 0;            // a continuing call (t_begin > 0) adds its launches to the same total

    // (a continuation keeps the status words: a give-up in an earlier slice must stay visible to wrnn_status(), and the
    // kernels leave at once when the abort flag is already up)
    if (pl.t0 == 0) HIPCHK(hipMemsetAsync(ws + l.status, 0, STATUS_WORDS * sizeof(unsigned), stream));
    // segment table -> device (pageable source: the runtime stages it before returning)
    HIPCHK(hipMemcpyAsync(ws + l.segs, seg_pos, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(ws + l.segs + (size_t)B * sizeof(int), seg_lim, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
    const int *d_pos = (const int *)(ws + l.segs), *d_lim = d_pos + B;
    if (o->mel_stage) {
        // the last up-sampling stage inside the loop: `mels_up` is that stage's input.  Everything is checked here, on the host: the
        // kernel reads rows j / s - 1 .. j / s + 1 without a bound.
        if (!k.mel_stage) { set_err("wrnn_options.mel_stage: only wrnn_duo_kernel / wrnn_sparse_kernel / wrnn_chain_kernel form the last up-sampling stage (this call runs on another kernel)"); return WRNN_ERR_ARG; }
        if (o->mel_stage != 1 || o->mel_scale != LAST_SCALE || !o->mel_taps || !o->seg_moff || o->mel_rows < 3) {
            set_err("wrnn_options.mel_stage=%d: needs mel_scale == %d (got %d), mel_taps, seg_moff, mel_rows >= 3", o->mel_stage, LAST_SCALE, o->mel_scale);
            return WRNN_ERR_ARG;
        }
        for (int b = 0; b < B; ++b) {
            const long last = (seg_lim[b] < (long)seg_pos[b] + T ? seg_lim[b] : (long)seg_pos[b] + T) - 1;      // last position that is not zero padding
            if (last < seg_pos[b]) continue;
            const long j0 = (long)seg_pos[b] + o->seg_moff[b], j1 = last + o->seg_moff[b];
            if (o->seg_moff[b] < 0 || j0 / LAST_SCALE < 1 || j1 / LAST_SCALE + 1 >= o->mel_rows) {
                set_err("segment %d: positions %ld..%ld of the last up-sampling stage reach outside its %d input rows", b, j0, j1, o->mel_rows);
                return WRNN_ERR_ARG;
            }
        }
        // out(q) = sum_j w[j] rep(q + j - s), rep(u) = in[u / s]: with q = s a + ph the taps j < s - ph fall on row a - 1, the next s on
        // row a, the last ph + 1 on row a + 1
        float coef[3 * LAST_SCALE];
        for (int ph = 0; ph < LAST_SCALE; ++ph) {
            double c0 = 0, c1 = 0, c2 = 0;
            for (int j = 0; j <= 2 * LAST_SCALE; ++j) {
                const double w = o->mel_taps[j];
                if (j < LAST_SCALE - ph) c0 += w; else if (j < 2 * LAST_SCALE - ph) c1 += w; else c2 += w;
            }
            coef[3 * ph] = (float)c0; coef[3 * ph + 1] = (float)c1; coef[3 * ph + 2] = (float)c2;
        }
        HIPCHK(hipMemcpyAsync(ws + l.segs + (size_t)2 * B * sizeof(int), o->seg_moff, (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
        HIPCHK(launch_put_floats((float *)(ws + l.melc), coef, 3 * LAST_SCALE, stream));       // (by value, as kernel arguments: `coef` is a stack array)
    }
    if (pl.kind == K_GENERIC || pl.kind == K_TILE || pl.kind == K_TILE_SPARSE || pl.kind == K_TILE_BF16 || pl.kind == K_TILE_WIDE) {
        GenArgs g;
        memset(&g, 0, sizeof g);
        g.I_T = p->g_I_T; g.I_b = p->I_b; g.w_ih1T = p->w_ih1T; g.w_hh1T = p->w_hh1T; g.b_ih1 = p->b_ih1; g.b_hh1 = p->b_hh1;
        g.w_ih2T = p->g_w_ih2T; g.w_hh2T = p->w_hh2T; g.b_ih2 = p->b_ih2; g.b_hh2 = p->b_hh2;
        g.fc1T = p->g_fc1T; g.fc1_b = p->fc1_b; g.fc2T = p->g_fc2T; g.fc2_b = p->fc2_b; g.fc3T = p->fc3T; g.fc3_b = p->fc3_b;
        g.mels_up = mels_up; g.aux = aux; g.noise = noise; g.force_x = o->force_x; g.out = out; g.dbg_logits = o->logits;
        g.seg_pos = d_pos; g.seg_lim = d_lim;
        if (lib_noise) {
            HIPCHK(launch_noise_fill(mol_mode, B, p->tr.C, 0, T, o->noise_seed, o->noise_seg_id, (float *)(ws + l.nlib), p->tr.n_cus, stream));
            g.noise = (const float *)(ws + l.nlib);
        }
        g.H = p->tr.gH; g.F = p->tr.gF; g.M = p->tr.gM; g.A = p->tr.gA; g.C = p->tr.C; g.B = B; g.T = T; g.hop = hop;
        if (watch) {        // every word = 0 = "nothing yet", on the stream in front of the launch
            HIPCHK(hipMemsetAsync(watch->progress, 0, (size_t)watch_need * sizeof(unsigned), stream));
            g.progress = watch->progress; g.progress_every = watch->every;
        }
        if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
        if (pl.kind == K_TILE_SPARSE && !p->ts_view) { set_err("this pack has no tile-sparse view"); return WRNN_ERR_ARG; }      // (the planner's traits are the pack's own: never)
        if (pl.kind == K_TILE_BF16 && !p->bf_bytes) { set_err("this pack has no bf16 view"); return WRNN_ERR_ARG; }             // (likewise)
        if (pl.kind == K_TILE_WIDE) {
            // a cooperative launch: W members per tile that cannot be co-resident are refused here, not hung
            const hipError_t e = launch_tile_wide(g, p->tr.mode, pl.ncl, ws + l.wide, (unsigned *)(ws + l.status), stream);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_err("%s cooperative launch failed: %s", k.name, hipGetErrorString(e));
                return e == hipErrorCooperativeLaunchTooLarge ? WRNN_ERR_RESIDENCY : WRNN_ERR_HIP;
            }
        } else
        HIPCHK(pl.kind == K_TILE_BF16   ? launch_tile_bf16(g, p->bf, p->tr.mode, stream)
               : pl.kind == K_TILE_SPARSE ? launch_tile_sparse(g, p->ts, p->tr.mode, p->ts_view == 2, stream)
               : pl.kind == K_TILE      ? launch_tile(g, p->tr.mode, stream)
                                        : launch_generic(g, p->tr.mode, stream));
        if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
        wrnn_run_info gi;
        memset(&gi, 0, sizeof gi);
        gi.kernel = k.name; gi.rounds = 1; gi.slab_steps = T; gi.launches = 1;
        if (pl.kind == K_TILE_WIDE) { gi.units_per_wg = k.units_per_wg; gi.clusters = pl.ncl; }
        if (o->info) *o->info = gi;
        return enqueue_progress(o, T, T, B, stream);
    }

    CondArgs c;
    memset(&c, 0, sizeof c);
    c.mels_up = mels_up; c.aux = aux; c.I_cT = p->I_cT; c.I_b = p->I_b; c.c2_wT = p->c2_wT; c.b_ih2 = p->b_ih2;
    c.c3_wT = p->c3_wT; c.fc1_b = p->fc1_b; c.c4_wT = p->c4_wT; c.fc2_b = p->fc2_b;
    c.c2f = (float *)(ws + l.c2f); c.c3f = (float *)(ws + l.c3f); c.c4f = (float *)(ws + l.c4f);
    c.seg_pos = d_pos; c.seg_lim = d_lim;
    c.B = B; c.T = T; c.hop = hop; c.NF = n_frames;
    if (k.slabbed) {
        // the aux tables are per segment and slab (filled in the slab loop): a slab may not span more than tab_fps - 2 whole hops
        const long eff = (long)(pl.tab_fps - 2) * hop + 1;
        if (pl.slab > eff) pl.slab = (int)eff;
    } else HIPCHK(launch_cond_frames(c, stream));

    LoopArgs a;
    memset(&a, 0, sizeof a);
    a.I_w0 = p->I_w0; a.w_ih1 = p->w_ih1; a.w_hh1 = p->w_hh1; a.b_ih1 = p->b_ih1; a.b_hh1 = p->b_hh1;
    a.w_ih2 = p->w_ih2; a.w_hh2 = p->w_hh2; a.b_hh2 = p->b_hh2; a.fc1_w = p->fc1_w; a.fc2_w = p->fc2_w;
    a.fc3_w = p->fc3_w; a.fc3_b = p->fc3_b; a.fc3f = p->fc3f; a.u1 = p->u1;
    a.w_ih1T = p->w_ih1T; a.w_hh1T = p->w_hh1T; a.w_ih2T = p->w_ih2T; a.w_hh2T = p->w_hh2T;
    a.fc1T = p->fc1T; a.fc2T = p->fc2T; a.fc3T = p->fc3T;
    a.c2f = c.c2f; a.c3f = c.c3f; a.c4f = c.c4f;
    a.noise = noise; a.force_x = o->force_x; a.out = out; a.dbg_logits = o->logits;
    a.status = (unsigned *)(ws + l.status);
    a.prof = (u64 *)o->phase_clocks;
    a.tuning = o->tuning;
    a.seg_pos = d_pos; a.seg_lim = d_lim;
    a.Btot = B; a.T = T; a.hop = hop; a.NF = n_frames; a.C = p->tr.C;
    a.NG = (B + SEG - 1) / SEG;
    a.Nall = B;
    a.xcc_tab = (unsigned *)(ws + l.xcc);
    a.mels_up = mels_up; a.aux_fr = aux; a.I_cT = p->I_cT; a.I_b = p->I_b;
    a.mel_stage = o->mel_stage; a.seg_moff = d_pos + 2 * B; a.mel_coef = (const float *)(ws + l.melc);
    hop_magic(hop, &a.hop_magic, &a.hop_shift);

    wrnn_run_info info;
    memset(&info, 0, sizeof info);
    info.kernel = k.name; info.units_per_wg = k.units_per_wg;
    info.clusters = pl.ncl; info.depth = pl.G; info.rounds = pl.rounds; info.slab_steps = pl.slab;

    if (k.persistent) {
        // ---- persistent loop kernels: for every slab of steps { derived noise; for every round { conditioning slab; loop } } ----
        a.sp_vals = p->sp_vals; a.sp_cols = p->sp_cols;
        a.sp_fc_vals = (o->tuning & 2048) ? nullptr : p->sp_fc_vals; a.sp_fc_cols = p->sp_fc_cols;      // (tuning bit 11: dense fc stages on a pack whose Linear layers are sparse too -- A/B)
        const bool mol = p->tr.mode == WRNN_MODE_MOL;
        a.xbuf = (float *)(ws + l.xbuf);
        a.cIf = (const float *)(ws + l.cIf);
        a.G = pl.G;
        c.cI = (float *)(ws + l.cIf);
        for (int s0 = pl.t0; s0 < pl.t1; s0 += pl.slab) {
            const int s1 = s0 + pl.slab < pl.t1 ? s0 + pl.slab : pl.t1;
            // wrnn_options.noise_lib: this slab's noise, drawn into the workspace in front of its launches -- what the caller's tensor holds in rows
            // [s0 - t_begin, s1 - t_begin)
            if (lib_noise) HIPCHK(launch_noise_fill(mol, B, p->tr.C, s0, s1, o->noise_seed, o->noise_seg_id, (float *)(ws + l.nlib), p->tr.n_cus, stream));
            // a slabbed kernel: derived noise, aux tables and the placement words of the slab's first launch in one launch (wrnn_slab_prep_kernel);
            // wrnn_options.tuning bit 13: by the three calls below, as before (A/B)
            const bool prep_fused = k.slabbed && !(o->tuning & 8192);
            const float *mol_rows = nullptr;
            if (mol) {   // noise rows are relative to t_begin (wrnn_options.t_begin)
                const float *const rows = lib_noise ? (const float *)(ws + l.nlib) : noise + (size_t)(s0 - pl.t0) * 11 * B;
                if (prep_fused) mol_rows = rows;
                else HIPCHK(launch_noise_mol(rows, (float *)(ws + l.npre), (long)(s1 - s0) * 11 * B, B, p->tr.n_cus, stream));
                a.noise_pre = (const float *)(ws + l.npre);
                a.noise_t0 = s0;
            } else if (lib_noise) {
                a.noise = (const float *)(ws + l.nlib);
                a.noise_t0 = s0;
            } else {
                a.noise_t0 = pl.t0;
            }
            if (k.slabbed) {   // this slab's aux tables of every segment of the call
                c.t0 = s0; c.B = B; c.FPS = pl.tab_fps;
                if (prep_fused) HIPCHK(launch_slab_prep(c, mol_rows, (float *)(ws + l.npre), (long)(s1 - s0) * 11 * B, (unsigned *)(ws + l.xcc), p->tr.n_cus, stream));
                else HIPCHK(launch_cond_frames_slab(c, stream));
                a.tab_fps = pl.tab_fps; a.tab_t0 = s0;
            }
            bool xcc_clear = prep_fused;      // (the placement words of the slab's FIRST launch are cleared by the prep kernel)
            for (int r = 0; r < pl.rounds; ++r) {
                const int rb0 = (int)(((long)r * B) / pl.rounds), rb1 = (int)(((long)(r + 1) * B) / pl.rounds);
                const int nr = rb1 - rb0;
                if (nr < 1) continue;
                const int ngr = (nr + SEG - 1) / SEG;
                c.t0 = s0; c.t1 = s1; c.rb0 = rb0; c.B = nr; c.NG = ngr;
                if (!k.slabbed) HIPCHK(launch_cond_frag(c, p->tr.n_cus, stream));
                // every word of the exchange ring = the sentinel.  A slabbed kernel leaves its ring consistent at the end of a launch
                // (every step re-arms the entries it will write two or three steps later), so it needs the fill only where a round starts: the first
                // launch of a call that starts at step 0, or any launch when several rounds share the buffer
                if (!k.slabbed || s0 == 0 || pl.rounds > 1 || (o->tuning & 4)) HIPCHK(hipMemsetAsync(ws + l.xbuf, 0xFF, k.xbuf_fill(pl.G), stream));
                if (k.slabbed && !xcc_clear) HIPCHK(hipMemsetAsync(ws + l.xcc, 0, XCC_WORDS * sizeof(unsigned), stream));      // placement handshake of this launch
                xcc_clear = false;
                a.state = (float *)(ws + l.state) + (size_t)r * k.state_floats(pl.G);
                a.t0 = s0; a.t1 = s1; a.cI_t0 = s0; a.rb0 = rb0; a.Btot = nr; a.NG = ngr; a.resume = s0 > 0 ? 1 : 0;
                a.kind_tag = k.kind_tag;
                if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
                hipError_t e = k.launch(a, pl.ncl, p->tr.sp_nbp, p->tr.mode, stream);
                // (two workgroups per CU not co-resident right now: WRNN_ERR_RESIDENCY -- the caller re-plans with WRNN_ALGO_LOOP, whose
                // workspace layout is another one: wavernn_amd/engine.py does)
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    set_err("%s cooperative launch failed: %s", info.kernel, hipGetErrorString(e));
                    return e == hipErrorCooperativeLaunchTooLarge ? WRNN_ERR_RESIDENCY : WRNN_ERR_HIP;
                }
                if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
                info.launches += 1;
            }
            if ((rc = enqueue_progress(o, s1, T, B, stream)) != WRNN_OK) return rc;
        }
    } else {
        // ---- stream kernel: whole-T conditioning in [t][segment][H] order, one launch --------------------
        c.cI = (float *)(ws + l.cI);
        a.cI = c.cI;
        HIPCHK(launch_cond(c, p->tr.n_cus, o->cond_valu != 0, stream));
        if (lib_noise) {
            HIPCHK(launch_noise_fill(mol_mode, B, p->tr.C, 0, T, o->noise_seed, o->noise_seg_id, (float *)(ws + l.nlib), p->tr.n_cus, stream));
            a.noise = (const float *)(ws + l.nlib);
        }
        a.b0 = 0;
        a.nb = B;
        if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
        HIPCHK(launch_stream(a, p->tr.mode, stream));
        if ((rc = timer_mark(timer, stream)) != WRNN_OK) return rc;
        info.launches = 1;
        if ((rc = enqueue_progress(o, T, T, B, stream)) != WRNN_OK) return rc;
    }
    if (o->info) *o->info = info;
    return WRNN_OK;
}

extern "C" int wrnn_generate_segments(const wrnn_pack *p, int32_t B, int32_t T, const int32_t *seg_pos,
                                      const int32_t *seg_lim, int32_t L, int32_t hop, int32_t n_frames,
                                      const float *mels_up, const float *aux, const float *noise, float *out,
                                      void *workspace, size_t workspace_bytes, const wrnn_options *opt, void *stream_)
{
    return generate_segments(p, B, T, seg_pos, seg_lim, L, hop, n_frames, mels_up, aux, noise, out, workspace, workspace_bytes, opt, stream_, nullptr);
}

extern "C" int wrnn_generate_segments_watched(const wrnn_pack *p, int32_t B, int32_t T, const int32_t *seg_pos,
                                              const int32_t *seg_lim, int32_t L, int32_t hop, int32_t n_frames,
                                              const float *mels_up, const float *aux, const float *noise, float *out,
                                              void *workspace, size_t workspace_bytes, const wrnn_options *opt, void *stream_,
                                              unsigned *progress, int32_t progress_words, int32_t progress_every)
{
    const Watch w = {progress, progress_words, progress_every};
    return generate_segments(p, B, T, seg_pos, seg_lim, L, hop, n_frames, mels_up, aux, noise, out, workspace, workspace_bytes, opt, stream_, &w);
}

extern "C" int wrnn_watch_words(const wrnn_pack *p, int32_t n_segments, int32_t T, const wrnn_options *opt, int32_t *words)
{
    if (!p || !words || n_segments < 1 || T < 1) { set_err("bad argument"); return WRNN_ERR_ARG; }
    int need = 0;
    const int rc = watch_check(&p->tr, n_segments, T, norm_struct(opt), nullptr, false, &need);
    if (rc == WRNN_OK) *words = need;
    return rc;
}

extern "C" int wrnn_debug_watch(const wrnn_plan_traits *traits, int32_t n_segments, int32_t T, const wrnn_options *opt, int32_t have_progress,
                                int32_t progress_words, int32_t progress_every, int32_t *words)
{
    if (!traits || n_segments < 1 || T < 1) { set_err("bad argument"); return WRNN_ERR_ARG; }
    const wrnn_plan_traits tr = norm_struct(traits);
    const Watch w = {nullptr, progress_words, progress_every};
    int need = 0;
    const int rc = watch_check(&tr, n_segments, T, norm_struct(opt), have_progress < 0 ? nullptr : &w, have_progress > 0, &need);
    if (rc == WRNN_OK && words) *words = need;
    return rc;
}

extern "C" int wrnn_generate(const wrnn_pack *p, const wrnn_geometry *g, const float *mels_up, const float *aux,
                             const float *noise, float *out, void *workspace, size_t workspace_bytes, const wrnn_options *opt,
                             void *stream_)
{
    int rc = check_geometry(g);
    if (rc != WRNN_OK) return rc;
    std::vector<int32_t> pos(g->B), lim(g->B, g->L);
    for (int b = 0; b < g->B; ++b) pos[b] = b * g->stride;
    return wrnn_generate_segments(p, g->B, g->T, pos.data(), lim.data(), g->L, g->hop, g->n_frames, mels_up, aux,
                                  noise, out, workspace, workspace_bytes, opt, stream_);
}

extern "C" int wrnn_status(void *workspace, void *stream)
{
    if (!workspace) { set_err("NULL workspace"); return WRNN_ERR_ARG; }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    unsigned st[STATUS_WORDS];
    HIPCHK(hipMemcpy(st, workspace, sizeof st, hipMemcpyDeviceToHost));
    if (st[0] != 0 || st[1] != 0) {
        set_err("loop kernel gave up: code 0x%x (phase %u) workgroup %u step %u thread %u", st[1], st[1] & 0xff, st[2], st[3], st[4]);
        return WRNN_ERR_KERNEL;
    }
    return WRNN_OK;
}

// Test hook: one exchanged layer (0 h1, 1 h2, 2 y1, 3 y2, 4 RAW logits) of (cluster, slot) at ring position `ring` of the loop
// kernel's exchange buffer, un-permuted from fragment order to host [16 segments][512].  Synchronises.
extern "C" int wrnn_debug_read_exchange(const wrnn_pack *p, void *workspace, int32_t n_segments, int32_t T, int32_t n_frames,
                                        const wrnn_options *opt, int cluster, int slot, int layer, int ring, float *host_out)
{
    if (!p || !workspace || !host_out) { set_err("NULL argument"); return WRNN_ERR_ARG; }
    const wrnn_options whole = whole_call(opt);
    Plan pl;
    int rc = make_plan(&p->tr, n_segments, T, &whole, &pl);
    if (rc != WRNN_OK) return rc;
    if (pl.kind != K_LOOP || cluster < 0 || cluster >= MAXCL || slot < 0 || slot >= LMAXG || layer < 0 || layer >= NXLAYER || ring < 0 || ring >= XRING) {
        set_err("no such exchange layer");
        return WRNN_ERR_ARG;
    }
    const WsLayout l = ws_layout(&p->tr, pl, n_segments, T, n_frames, whole.noise_lib != 0);
    HIPCHK(hipDeviceSynchronize());
    std::vector<float> frag((size_t)SEG * H);
    const size_t off = ((((size_t)cluster * LMAXG + slot) * NXLAYER + layer) * XRING + ring) * SEG * H;
    HIPCHK(hipMemcpy(frag.data(), (char *)workspace + l.xbuf + off * sizeof(float), frag.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int j = 0; j < SEG; ++j)
        for (int k = 0; k < H; ++k) {
            const int w = k >> 7, r = (k >> 4) & 7, kq = (k >> 2) & 3, e = k & 3;
            host_out[(size_t)j * H + k] = frag[(size_t)(((w * 8 + r) * 64 + kq * 16 + j) * 4 + e)];
        }
    return WRNN_OK;
}

namespace {
int check_noise_fill(int mode, int32_t B, int32_t C, int32_t t0, int32_t t1, const float *out)
{
    if (mode != WRNN_MODE_MOL && mode != WRNN_MODE_RAW) { set_err("unknown mode %d", mode); return WRNN_ERR_ARG; }
    if (!out) { set_err("NULL argument"); return WRNN_ERR_ARG; }
    if (B < 1 || t0 < 0 || t1 <= t0 || (mode == WRNN_MODE_RAW && C < 1)) { set_err("bad noise shape: %d segments, %d classes, steps [%d, %d)", B, C, t0, t1); return WRNN_ERR_ARG; }
    if ((double)(t1 - t0) * B >= 2147483648.0) { set_err("%d steps x %d segments: more than 2^31 - 1 rows in one fill; split the step range", t1 - t0, B); return WRNN_ERR_ARG; }
    return WRNN_OK;
}
}  // namespace

extern "C" int wrnn_noise_fill(int mode, int32_t n_segments, int32_t n_classes, int32_t t_begin, int32_t t_end, uint64_t seed, const uint64_t *seg_id,
                               float *out, int device, void *stream)
{
    int rc = check_noise_fill(mode, n_segments, n_classes, t_begin, t_end, out);
    if (rc != WRNN_OK) return rc;
    if (((uintptr_t)out & 15) != 0) { set_err("`out` must be 16-byte aligned"); return WRNN_ERR_ARG; }
    const int cus = wrnn_device_cus(device);
    if (cus < 0) return cus;
    DeviceGuard dg(device);
    HIPCHK(dg.err);
    HIPCHK(launch_noise_fill(mode == WRNN_MODE_MOL, n_segments, n_classes, t_begin, t_end, seed, seg_id, out, cus, (hipStream_t)stream));
    return WRNN_OK;
}

extern "C" int wrnn_noise_fill_host(int mode, int32_t n_segments, int32_t n_classes, int32_t t_begin, int32_t t_end, uint64_t seed, const uint64_t *seg_id,
                                    float *out)
{
    const int rc = check_noise_fill(mode, n_segments, n_classes, t_begin, t_end, out);
    if (rc != WRNN_OK) return rc;
    noise_fill_host(mode == WRNN_MODE_MOL, n_segments, n_classes, t_begin, t_end, seed, seg_id, out);
    return WRNN_OK;
}

namespace {
int check_nll(const wrnn_nll_call *c)
{
    if (!c) { set_err("NULL wrnn_nll_call"); return WRNN_ERR_ARG; }
    if (c->struct_bytes != sizeof(wrnn_nll_call)) { set_err("wrnn_nll_call.struct_bytes is %u, this library's struct has %zu bytes", c->struct_bytes, sizeof(wrnn_nll_call)); return WRNN_ERR_ARG; }
    if (!c->logits || !c->target || !c->sum) { set_err("NULL %s", !c->logits ? "logits" : !c->target ? "target" : "sum"); return WRNN_ERR_ARG; }
    if (c->mode != WRNN_MODE_MOL && c->mode != WRNN_MODE_RAW) { set_err("unknown mode %d", c->mode); return WRNN_ERR_ARG; }
    if (c->mode == WRNN_MODE_MOL && c->n_classes != 30) { set_err("MOL scores 30 outputs per step (10 mixtures), not %d", c->n_classes); return WRNN_ERR_ARG; }
    if (c->mode == WRNN_MODE_RAW && (c->n_classes < 2 || c->n_classes > 2048)) { set_err("RAW scores 2..2048 classes, not %d", c->n_classes); return WRNN_ERR_ARG; }
    if (c->n_segments < 1 || c->T < 1) { set_err("bad shape: %d segments, %d steps", c->n_segments, c->T); return WRNN_ERR_ARG; }
    return WRNN_OK;
}
NllArgs nll_args(const wrnn_nll_call *c) { return NllArgs{c->logits, c->target, c->seg_len, c->nll, c->sum, c->n_segments, c->T, c->n_classes}; }
}  // namespace

extern "C" int wrnn_nll(int device, const wrnn_nll_call *c)
{
    const int rc = check_nll(c);
    if (rc != WRNN_OK) return rc;
    const int cus = wrnn_device_cus(device);
    if (cus < 0) return cus;
    DeviceGuard dg(device);
    HIPCHK(dg.err);
    HIPCHK(launch_nll(c->mode == WRNN_MODE_MOL, nll_args(c), (hipStream_t)c->stream));
    return WRNN_OK;
}

extern "C" int wrnn_nll_host(const wrnn_nll_call *c)
{
    const int rc = check_nll(c);
    if (rc != WRNN_OK) return rc;
    nll_host(c->mode == WRNN_MODE_MOL, nll_args(c));
    return WRNN_OK;
}

// Test hook: the launch planner on a description of pack and device -- make_plan + ws_layout, as wrnn_plan_segments and
// wrnn_workspace_bytes_segments run them on a pack's own traits -- without a pack, a device or the HIP runtime.
extern "C" int wrnn_debug_plan(const wrnn_plan_traits *traits, int32_t n_segments, int32_t T, int32_t n_frames,
                               const wrnn_options *opt, wrnn_run_info *out, size_t *workspace_bytes)
{
    if (!traits || !out || !workspace_bytes || n_segments < 1 || T < 1 || n_frames < 1) { set_err("bad argument"); return WRNN_ERR_ARG; }
    *workspace_bytes = 0;
    const wrnn_plan_traits tr = norm_struct(traits);
    return plan_report(&tr, n_segments, T, n_frames, norm_struct(opt), out, workspace_bytes);      // (the step range stays: validated as for wrnn_generate_segments)
}

static float g_selftest_metric = -1.f;
extern "C" float wrnn_selftest_metric(void) { return g_selftest_metric; }

extern "C" int wrnn_selftest(int device, int which)
{
    const int cus = wrnn_device_cus(device);
    if (cus < 0) return cus;
    DeviceGuard dg(device);
    HIPCHK(dg.err);
    char msg[400] = "";
    int rc;
    if (which == 1) rc = selftest_mfma(msg, sizeof msg);
    else if (which == 2) rc = selftest_allgather(cus, msg, sizeof msg, &g_selftest_metric);
    else if (which == 3) rc = selftest_tanh(msg, sizeof msg);
    else if (which == 4) rc = selftest_xor(msg, sizeof msg);
    else { set_err("unknown selftest %d", which); return WRNN_ERR_ARG; }
    if (rc != 0) { set_err("selftest %d failed: %s", which, msg); return WRNN_ERR_KERNEL; }
    set_err("selftest %d ok: %s", which, msg);
    return WRNN_OK;
}
