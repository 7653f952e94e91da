// BARE's batch-statistics pruning, forward (deep-learning/methods/train_bare.py:28-57, WeightedCCE.forward).
//
// With p = clamp(softmax(z), 1e-8, 1 - 1e-8) (:33-34), pt_i = p[i, y_i] (:35), mu_c the batch mean of column c (:38)
// and sd_c its unbiased deviation (:40, torch.std: the divisor is B - 1, NaN for B = 1), row i is kept when
//     pt_i - mu[y_i] >= k * sd[y_i]                                                          (:42-45, :49)
// and L = the mean cross-entropy (on the raw logits) of the kept rows (:51-53); if no row is kept, L = the mean
// cross-entropy of all rows (:55, the fallback, whatever `reduction` says).  The statistics carry no gradient: they
// only choose rows, so dL/dz_i = w_i (softmax(z_i) - e_y) with w_i = 1 / n_kept on the kept rows and 0 elsewhere
// (1 / B everywhere in the fallback).  In fp32 the upper clamp is 1.0f and does nothing; the lower one is applied.
//
// The row kernels of this library reduce along a row; here every softmax COLUMN needs its sum and sum of squares down
// the batch before any row can be judged.  Column sums are fixed-point integers: p and p^2 quantised to 2^-40 (p <= 1,
// B <= 2^22: no overflow in 64 bits), so they add exactly in any order -- per lane in registers, per workgroup with
// LDS integer adds, over the workgroups' slabs in the finish kernel -- and every run gives the same bits.  The
// deviation comes from B * S2 * 2^40 - S1^2 as an exact 128-bit integer: no subtraction of rounded numbers.
//
// Streaming form, launches only, no host round trip:
//   pass 1 (bare_rows_kernel): reads the block once; per row max, log-sum-exp, CE_i, pt_i, the top-1 hit and the label
//     check; per column the integer sums of p and p^2 over the workgroup's rows, written as one slab per workgroup
//     {S1[C], S2[C], hits, 0} (written whole before it is read: the region needs no initial value);
//   finish (bare_finish_kernel, one workgroup): slabs -> mu[C], sd[C]; judges every row, counts, forms L, writes
//     w, sel and out = {L, n_kept, fallback, 100 * hits / B};
//   the gradient is the streaming M-step entry with weights = w, idx = NULL, inv_scale = 1 (no kernel of its own).
// One-workgroup form (bare_small_kernel): B * C <= 16 384 with B <= 1024 and C <= 1024 -- the reference's own batches
//   (32 x 10, 128 x 10, 128 x 100), where three launches are all latency: the same row arithmetic (the same template,
//   so pt, mu, sd and therefore sel are bit-identical to the streaming form's), the softmax block kept in LDS, the
//   statistics, the selection, L and the gradient w_i (softmax - e_y) in ONE launch.
// A row lives in the registers of a group of G lanes: lane g holds the V-element vectors k * G + g, k < NK.
#include "rlvi_common.h"

namespace rlvi {

constexpr int BR_THREADS = 256;               // pass 1
constexpr int BR_WAVES = BR_THREADS / WAVE;
constexpr int BF_THREADS = 1024;              // finish, and the one-workgroup form
constexpr int BF_WAVES = BF_THREADS / WAVE;
constexpr int BARE_MAX_C = 4096;
constexpr int64_t BARE_MAX_B = (int64_t)1 << 22;
constexpr int64_t BARE_SMALL_ELEMS = 16384;   // one-workgroup form: B * C up to this, B and C up to BARE_SMALL_DIM
constexpr int BARE_SMALL_DIM = 1024;
constexpr size_t BARE_LDS_ASK = 60 * 1024;      // dynamic LDS beyond this (with the static arrays: 64 KiB) is asked for
constexpr float BARE_EPS = 1e-8f;
constexpr double BARE_FIX = 1099511627776.0;  // 2^40
typedef unsigned long long u64;

__device__ __forceinline__ float bare_clamp(float p) { return fminf(fmaxf(p, BARE_EPS), 1.0f - BARE_EPS); }
__device__ __forceinline__ u64 bare_fix1(float p) { return __float2ull_rn(p * 1099511627776.0f); }
__device__ __forceinline__ u64 bare_fix2(float p) { return __double2ull_rn((double)p * (double)p * BARE_FIX); }

// One row in the registers of G lanes.  After stats(): d = z - max (dead slots -inf), s = sum exp(d), r1 = 1 / s.
template <typename T, int V, int G, int NK>
struct BareRow {
    float d[NK][V];
    bool live[NK];
    float m, s, ls, r1;
    int earlier;                 // columns before y that attain the maximum

    __device__ __forceinline__ void load(const T *zr, int C, int g) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int col = (k * G + g) * V;
            live[k] = col < C;                                   // V divides C: a vector is inside or outside
            VecIO<T, V>::load(zr + (live[k] ? col : 0), d[k]);   // dead slots re-read the first vector
        }
    }
    __device__ __forceinline__ void stats(int g, int y) {
        const float NEG_INF = -__builtin_inff();
        float mx = NEG_INF;
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                d[k][j] = live[k] ? d[k][j] : NEG_INF;
                mx = fmaxf(mx, d[k][j]);
            }
        m = group_max<G>(mx);
        float a = 0.0f;
        int ea = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                d[k][j] -= m;
                a += mexp(d[k][j]);
                ea += (d[k][j] == 0.0f && (k * G + g) * V + j < y) ? 1 : 0;
            }
        s = group_sum<G>(a);
        earlier = group_allreduce<G>(ea, FAdd());
        ls = logf(s);
        r1 = 1.0f / s;
    }
    __device__ __forceinline__ float prob(int k, int j) const { return mexp(d[k][j]) * r1; }
    // the label's column from its own load (every lane of the group): CE as torch evaluates it, pt clamped
    __device__ __forceinline__ float ce(float zy) const { return ls - (zy - m); }
    __device__ __forceinline__ float pt(float zy) const { return bare_clamp(mexp(zy - m) * r1); }
};

// mu and sd of one column from its exact integer sums S1 = sum fix(p), S2 = sum fix(p^2) (units of 2^-40).
__device__ __forceinline__ void bare_mu_sd(u64 S1, u64 S2, int64_t B, float &mu, float &sd) {
    mu = (float)((double)S1 / (BARE_FIX * (double)B));
    if (B < 2) { sd = __builtin_nanf(""); return; }
    // B * sum p^2 - (sum p)^2 in units of 2^-80, exactly: both terms stay below 2^124
    const unsigned __int128 a = ((unsigned __int128)S2 * (u64)B) << 40;
    const unsigned __int128 b = (unsigned __int128)S1 * S1;
    double var = 0.0;                                // (the two quantisations may leave a - b a hair below zero)
    if (a > b) {
        const unsigned __int128 dlt = a - b;
        const double x = (double)(u64)(dlt >> 64) * 18446744073709551616.0 + (double)(u64)dlt;
        var = x / (BARE_FIX * BARE_FIX) / ((double)B * (double)(B - 1));
    }
    sd = (float)sqrt(var);
}

// the reference's comparison, in its fp32 rounding order; false for a NaN (B = 1, a label out of range)
__device__ __forceinline__ bool bare_keep(float pt, float mu, float sd, float k) {
    return __fsub_rn(pt, mu) >= __fmul_rn(k, sd);
}

// ---- pass 1 -------------------------------------------------------------------------------------------------
// ce_out / pt_out are the caller's w / sel vectors: the finish kernel reads them and writes the results over them.
template <typename T, int V, int G, int NK>
__global__ __launch_bounds__(BR_THREADS) void bare_rows_kernel(const T *__restrict__ z, int64_t ld,
                                                               const int64_t *__restrict__ labels, int64_t B, int C,
                                                               float *__restrict__ ce_out, float *__restrict__ pt_out,
                                                               u64 *__restrict__ slab, int32_t *__restrict__ status) {
    extern __shared__ u64 sh[];                      // S1[C], S2[C], hits, 0
    constexpr int R = WAVE / G;
    constexpr bool REG = NK * V <= 16;               // column sums in registers over the row loop, else LDS adds per row
    constexpr int NA = REG ? NK : 1;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int g = lane & (G - 1), sub = lane / G;
    const int n = 2 * C + 2;
    for (int i = threadIdx.x; i < n; i += BR_THREADS) sh[i] = 0;
    __syncthreads();
    u64 a1[NA][V], a2[NA][V];
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) a1[k][j] = a2[k][j] = 0;
    u64 hits = 0;
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * BR_WAVES * R;
    for (int64_t row0 = ((int64_t)blockIdx.x * BR_WAVES + wave) * R; row0 < B; row0 += stride) {
        const int64_t row = row0 + sub;
        const bool valid = row < B;
        const int64_t rr = valid ? row : B - 1;      // padding rows recompute the last row, count nothing
        const int64_t y64 = labels[rr];
        BareRow<T, V, G, NK> r;
        r.load(z + rr * ld, C, g);
        const bool y_ok = y64 >= 0 && y64 < C;
        bad = bad || (valid && !y_ok);
        const int y = y_ok ? (int)y64 : 0;
        const float zy = load1(z + rr * ld, y);
        r.stats(g, y);
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int col = (k * G + g) * V;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float p = bare_clamp(r.prob(k, j));
                const bool on = valid && r.live[k];
                if (REG) {
                    a1[k % NA][j] += on ? bare_fix1(p) : 0ull;
                    a2[k % NA][j] += on ? bare_fix2(p) : 0ull;
                } else if (on) {
                    atomicAdd(&sh[col + j], bare_fix1(p));
                    atomicAdd(&sh[C + col + j], bare_fix2(p));
                }
            }
        }
        if (g == 0 && valid) {
            // a label out of range: the row is never kept and adds nothing to L
            ce_out[row] = y_ok ? r.ce(zy) : 0.0f;
            pt_out[row] = y_ok ? r.pt(zy) : __builtin_nanf("");
            hits += (y_ok && zy == r.m && r.earlier == 0) ? 1 : 0;
        }
    }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    if (REG) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int col = (k * G + g) * V;
            if (col < C) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    atomicAdd(&sh[col + j], a1[k][j]);
                    atomicAdd(&sh[C + col + j], a2[k][j]);
                }
            }
        }
    }
    hits = wave_sum(hits);
    if (lane == 0) atomicAdd(&sh[2 * C], hits);
    __syncthreads();
    u64 *mine = slab + (size_t)blockIdx.x * n;
    for (int i = threadIdx.x; i < n; i += BR_THREADS) mine[i] = sh[i];
}

// Fixed-order sum of three per-thread doubles over a workgroup of BF_THREADS threads; the totals in every thread.
__device__ __forceinline__ void bare_block_sum3(double &a, double &b, double &c, double *shd) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    a = wave_sum(a);
    b = wave_sum(b);
    c = wave_sum(c);
    __syncthreads();
    if (lane == 0) { shd[3 * wave] = a; shd[3 * wave + 1] = b; shd[3 * wave + 2] = c; }
    __syncthreads();
    a = b = c = 0.0;
    for (int w = 0; w < BF_WAVES; ++w) { a += shd[3 * w]; b += shd[3 * w + 1]; c += shd[3 * w + 2]; }
}

// ---- finish: one workgroup ----------------------------------------------------------------------------------
__global__ __launch_bounds__(BF_THREADS) void bare_finish_kernel(const u64 *__restrict__ slab, int nslab,
                                                                 const int64_t *__restrict__ labels, int64_t B, int C,
                                                                 float k, float *__restrict__ w,
                                                                 float *__restrict__ sel, float *__restrict__ out) {
    extern __shared__ u64 tot[];                     // S1[C], S2[C], hits, 0; then mu[C], sd[C] as fp32
    __shared__ double shd[3 * BF_WAVES];
    const int tid = threadIdx.x;
    const int n = 2 * C + 2;
    float *mu = reinterpret_cast<float *>(tot + n), *sd = mu + C;
    for (int i = tid; i < n; i += BF_THREADS) tot[i] = 0;
    __syncthreads();
    // thread t sums entry t % n of the slabs t / n, t / n + P, ...: integer adds, any order gives the same bits
    const int P = BF_THREADS / n > 0 ? BF_THREADS / n : 1;
    for (int e = tid; e < n * P; e += BF_THREADS) {
        const int c = e % n;
        u64 acc = 0;
        for (int s = e / n; s < nslab; s += P) acc += slab[(size_t)s * n + c];
        atomicAdd(&tot[c], acc);
    }
    __syncthreads();
    for (int c = tid; c < C; c += BF_THREADS) bare_mu_sd(tot[c], tot[C + c], B, mu[c], sd[c]);
    __syncthreads();
    double cnt = 0.0, sum_kept = 0.0, sum_all = 0.0;
    for (int64_t i = tid; i < B; i += BF_THREADS) {
        const int64_t y = labels[i];
        const float pt = sel[i], ce = w[i];
        const bool keep = y >= 0 && y < C && bare_keep(pt, mu[y], sd[y], k);
        sel[i] = keep ? 1.0f : 0.0f;
        cnt += keep ? 1.0 : 0.0;
        sum_kept += keep ? (double)ce : 0.0;
        sum_all += (double)ce;
    }
    bare_block_sum3(cnt, sum_kept, sum_all, shd);
    const bool fallback = cnt == 0.0;
    const double nk = fallback ? (double)B : cnt;
    const float wv = 1.0f / (float)nk;
    for (int64_t i = tid; i < B; i += BF_THREADS) {  // thread tid wrote sel[i] above
        const bool keep = fallback || sel[i] != 0.0f;
        sel[i] = keep ? 1.0f : 0.0f;
        w[i] = keep ? wv : 0.0f;
    }
    if (tid == 0) {
        out[0] = (float)((fallback ? sum_all : sum_kept) / nk);
        out[1] = (float)nk;
        out[2] = fallback ? 1.0f : 0.0f;
        out[3] = (float)((double)tot[2 * C] * 100.0 / (double)B);
    }
}

// ---- one-workgroup form ---------------------------------------------------------------------------------------
// LDS: S1[C], S2[C] (u64); the softmax block [B][C], mu[C], sd[C], per row CE, pt, w (fp32) and the label (int).
__host__ __device__ inline size_t bare_small_lds(int64_t B, int64_t C) {
    return (size_t)(2 * C) * 8 + (size_t)(B * C + 2 * C + 4 * B) * 4;
}

template <typename T, int V, int G, int NK>
__global__ __launch_bounds__(BF_THREADS) void bare_small_kernel(const T *__restrict__ z, int64_t ld,
                                                                const int64_t *__restrict__ labels, int B, int C,
                                                                float k, float *__restrict__ w,
                                                                float *__restrict__ sel, float *__restrict__ out,
                                                                T *__restrict__ grad, int64_t ldg, int gvec,
                                                                int32_t *__restrict__ status) {
    extern __shared__ u64 tot[];
    __shared__ double shd[3 * BF_WAVES];
    __shared__ int sh_hits;
    constexpr int R = WAVE / G;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int g = lane & (G - 1), sub = lane / G;
    float *pb = reinterpret_cast<float *>(tot + 2 * C);
    float *mu = pb + (size_t)B * C, *sd = mu + C;
    float *row_ce = sd + C, *row_pt = row_ce + B, *row_w = row_pt + B;
    int *row_y = reinterpret_cast<int *>(row_w + B);
    for (int i = tid; i < 2 * C; i += BF_THREADS) tot[i] = 0;
    if (tid == 0) sh_hits = 0;
    __syncthreads();
    bool bad = false;
    int hits = 0;
    for (int row0 = wave * R; row0 < B; row0 += BF_WAVES * R) {
        const int row = row0 + sub;
        const bool valid = row < B;
        const int rr = valid ? row : B - 1;
        const int64_t y64 = labels[rr];
        BareRow<T, V, G, NK> r;
        r.load(z + (int64_t)rr * ld, C, g);
        const bool y_ok = y64 >= 0 && y64 < C;
        bad = bad || (valid && !y_ok);
        const int y = y_ok ? (int)y64 : 0;
        const float zy = load1(z + (int64_t)rr * ld, y);
        r.stats(g, y);
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
            const int col = (kk * G + g) * V;
            if (valid && r.live[kk]) {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float p = r.prob(kk, j);
                    pb[(size_t)row * C + col + j] = p;
                    atomicAdd(&tot[col + j], bare_fix1(bare_clamp(p)));
                    atomicAdd(&tot[C + col + j], bare_fix2(bare_clamp(p)));
                }
            }
        }
        if (g == 0 && valid) {
            row_ce[row] = y_ok ? r.ce(zy) : 0.0f;
            row_pt[row] = y_ok ? r.pt(zy) : __builtin_nanf("");
            row_y[row] = y_ok ? y : -1;
            hits += (y_ok && zy == r.m && r.earlier == 0) ? 1 : 0;
        }
    }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    hits = wave_sum(hits);
    if (lane == 0) atomicAdd(&sh_hits, hits);
    __syncthreads();
    for (int c = tid; c < C; c += BF_THREADS) bare_mu_sd(tot[c], tot[C + c], B, mu[c], sd[c]);
    __syncthreads();
    // thread i judges row i (B <= BF_THREADS)
    const int y = tid < B ? row_y[tid] : -1;
    const bool keep = y >= 0 && bare_keep(row_pt[tid < B ? tid : 0], mu[y >= 0 ? y : 0], sd[y >= 0 ? y : 0], k);
    const float ce = tid < B ? row_ce[tid] : 0.0f;
    double cnt = keep ? 1.0 : 0.0, sum_kept = keep ? (double)ce : 0.0, sum_all = (double)ce;
    bare_block_sum3(cnt, sum_kept, sum_all, shd);
    const bool fallback = cnt == 0.0;
    const double nk = fallback ? (double)B : cnt;
    const float wv = 1.0f / (float)nk;
    if (tid < B) {
        const bool kp = fallback || keep;
        sel[tid] = kp ? 1.0f : 0.0f;
        w[tid] = kp ? wv : 0.0f;
        row_w[tid] = (kp && y >= 0) ? wv : 0.0f;     // a label out of range: a zero gradient row, as the M-step's
    }
    if (tid == 0) {
        out[0] = (float)((fallback ? sum_all : sum_kept) / nk);
        out[1] = (float)nk;
        out[2] = fallback ? 1.0f : 0.0f;
        out[3] = (float)((double)sh_hits * 100.0 / (double)B);
    }
    if (grad == nullptr) return;
    __syncthreads();
    const int nv = C / V;                            // vectors per row
    for (int e = tid; e < B * nv; e += BF_THREADS) {
        const int row = e / nv, col = (e - row * nv) * V;
        const float wr = row_w[row];
        const int yr = row_y[row];
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = wr * (pb[(size_t)row * C + col + j] - (col + j == yr ? 1.0f : 0.0f));
        if (gvec) {
            VecIO<T, V>::store(grad + (int64_t)row * ldg + col, o);
        } else {                                     // a gradient block whose rows are not vector-aligned
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float o1[1] = {o[j]};
                VecIO<T, 1>::store(grad + (int64_t)row * ldg + col + j, o1);
            }
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------
// the row shapes: G lanes x NK vectors of V elements hold a row of up to G * NK * V elements
struct BareShape {
    int V, G, NK;
};

template <typename T>
static BareShape bare_pick_shape(const void *z, int64_t ld, int64_t C) {
    const bool v4 = vec_fits<T>(4, C, {{z, ld}});    // from the logits alone: both forms take the same shape
    if (v4) {
        if (C <= 16) return {4, 4, 1};
        if (C <= 64) return {4, 16, 1};
        if (C <= 256) return {4, 16, 4};
        if (C <= 1024) return {4, 64, 4};
        return {4, 64, 16};
    }
    if (C <= 16) return {1, 4, 4};
    if (C <= 64) return {1, 16, 4};
    if (C <= 256) return {1, 64, 4};
    if (C <= 1024) return {1, 64, 16};
    return {1, 64, 64};
}

// Which form a call takes: 1 one workgroup, 0 streaming.  RLVI_BARE_FORM: -1 by size, 0 streaming, 1 one workgroup
// wherever it can hold the block at all.
static int bare_form(int64_t B, int64_t C) {
    const bool can = B * C <= BARE_SMALL_ELEMS && B <= BARE_SMALL_DIM && C <= BARE_SMALL_DIM;
    const int knob = tune_get("RLVI_BARE_FORM", -1);
    return knob == 0 ? 0 : can ? 1 : 0;
}

#define RLVI_BARE_SHAPES(X, sh)                                  \
    if (sh.V == 4) {                                             \
        if (sh.G == 4) X(4, 4, 1);                               \
        else if (sh.G == 16 && sh.NK == 1) X(4, 16, 1);          \
        else if (sh.G == 16) X(4, 16, 4);                        \
        else if (sh.NK == 4) X(4, 64, 4);                        \
        else X(4, 64, 16);                                       \
    } else {                                                     \
        if (sh.G == 4) X(1, 4, 4);                               \
        else if (sh.G == 16) X(1, 16, 4);                        \
        else if (sh.NK == 4) X(1, 64, 4);                        \
        else if (sh.NK == 16) X(1, 64, 16);                      \
        else X(1, 64, 64);                                       \
    }
#define RLVI_BARE_SMALL_SHAPES(X, sh)                            \
    if (sh.V == 4) {                                             \
        if (sh.G == 4) X(4, 4, 1);                               \
        else if (sh.G == 16 && sh.NK == 1) X(4, 16, 1);          \
        else if (sh.G == 16) X(4, 16, 4);                        \
        else X(4, 64, 4);                                        \
    } else {                                                     \
        if (sh.G == 4) X(1, 4, 4);                               \
        else if (sh.G == 16) X(1, 16, 4);                        \
        else if (sh.NK == 4) X(1, 64, 4);                        \
        else X(1, 64, 16);                                       \
    }

template <typename T>
static int bare_fwd(const T *z, int64_t ld, const int64_t *labels, int64_t B, int64_t C, float k, float *w, float *sel,
                    float *out, T *grad, int64_t ldg, void *ws, void *stream) {
    if (!z || !labels || !w || !sel || !out || !ws) return RLVI_E_NULL;
    if (B <= 0 || C <= 0 || ld < C || (grad && ldg < C) || k != k) return RLVI_E_SHAPE;
    if (C > BARE_MAX_C || B > BARE_MAX_B) return RLVI_E_LIMIT;
    if (((uintptr_t)labels & 7) || ((uintptr_t)w & 3) || ((uintptr_t)sel & 3) || ((uintptr_t)out & 3) ||
        ((uintptr_t)ws & 255) || ((uintptr_t)z % sizeof(T)) || ((uintptr_t)grad % sizeof(T)))
        return RLVI_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    int32_t *status = reinterpret_cast<int32_t *>(base);
    const int Ci = (int)C;
    int rc = 0;
    if (bare_form(B, C) == 1) {
        const BareShape sh = bare_pick_shape<T>(z, ld, C);
        const int gvec = vec_fits<T>(sh.V, C, {{grad, ldg}}) ? 1 : 0;
        const size_t lds = bare_small_lds(B, C);
#define RLVI_BS(V_, G_, NK_)                                                                               \
    do {                                                                                                   \
        auto kern = bare_small_kernel<T, V_, G_, NK_>;                                                     \
        if (lds > BARE_LDS_ASK) rc = allow_dyn_lds(kern, lds);                                                    \
        if (!rc)                                                                                           \
            rc = launch(kern, dim3(1), dim3(BF_THREADS), lds, st, z, ld, labels, (int)B, Ci, k, w, sel, out, grad, \
                        ldg, gvec, status);                                                                    \
    } while (0)
        RLVI_BARE_SMALL_SHAPES(RLVI_BS, sh)
#undef RLVI_BS
        return rc;
    }
    // the slabs live in the weighted-least-squares region of the workspace (256 KiB, needs no initial value, and a
    // workspace serves one stream at a time): as many workgroups as slabs of 2C + 2 words fit, at most 1024
    u64 *slab = reinterpret_cast<u64 *>(base + WS_WLS_OFF);
    const int64_t n = 2 * C + 2;
    const BareShape sh = bare_pick_shape<T>(z, ld, C);
    const int rows_per_block = BR_WAVES * (WAVE / sh.G);
    int64_t nb = (B + rows_per_block - 1) / rows_per_block;
    const int64_t fit = (int64_t)(WS_WLS_BYTES / 8) / n;
    if (nb > fit) nb = fit;
    if (nb > MSTEP_MAX_BLOCKS) nb = MSTEP_MAX_BLOCKS;
    const size_t lds1 = (size_t)n * 8;
    const size_t lds2 = (size_t)n * 8 + (size_t)(2 * C) * 4;
#define RLVI_BR(V_, G_, NK_)                                                                                       \
    do {                                                                                                           \
        auto kern = bare_rows_kernel<T, V_, G_, NK_>;                                                              \
        if (lds1 > BARE_LDS_ASK) rc = allow_dyn_lds(kern, lds1);                                                          \
        if (!rc)                                                                                                   \
            rc = launch(kern, dim3((unsigned)nb), dim3(BR_THREADS), lds1, st, z, ld, labels, B, Ci, w, sel, slab, status); \
    } while (0)
    RLVI_BARE_SHAPES(RLVI_BR, sh)
#undef RLVI_BR
    if (rc) return rc;
    if (lds2 > BARE_LDS_ASK) rc = allow_dyn_lds(bare_finish_kernel, lds2);
    if (rc) return rc;
    return launch(bare_finish_kernel, dim3(1), dim3(BF_THREADS), lds2, st, slab, (int)nb, labels, B, Ci, k, w, sel, out);
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_bare_form(int64_t B, int64_t C) {
    if (B <= 0 || C <= 0) return RLVI_E_SHAPE;
    if (C > BARE_MAX_C || B > BARE_MAX_B) return RLVI_E_LIMIT;
    return bare_form(B, C);
}

extern "C" int rlvi_bare_fwd_f32(const float *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C, float k,
                                 float *w, float *sel, float *out, float *grad, int64_t ldg, void *ws, void *stream) {
    return bare_fwd<float>(logits, ld, labels, B, C, k, w, sel, out, grad, ldg, ws, stream);
}
extern "C" int rlvi_bare_fwd_bf16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C,
                                  float k, float *w, float *sel, float *out, uint16_t *grad, int64_t ldg, void *ws,
                                  void *stream) {
    return bare_fwd<uint16_t>(logits, ld, labels, B, C, k, w, sel, out, grad, ldg, ws, stream);
}
extern "C" int rlvi_bare_fwd_f16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C,
                                 float k, float *w, float *sel, float *out, uint16_t *grad, int64_t ldg, void *ws,
                                 void *stream) {
    return bare_fwd<f16_t>(reinterpret_cast<const f16_t *>(logits), ld, labels, B, C, k, w, sel, out,
                           reinterpret_cast<f16_t *>(grad), ldg, ws, stream);
}
