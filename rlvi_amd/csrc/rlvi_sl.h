// What the one-workgroup fp64 estimators (standard.hip: linear regression, the online weights; logreg.hip: logistic
// regression; moments.hip: mean, PCA, covariance, the constrained E-step) share, ONE copy of each piece:
//   * the workgroup's shape, the reciprocal, the lane broadcast;
//   * the block reductions (sl_block_sum<K>, sl_block_max, sl_block_minmax) on parity-buffered LDS slots;
//   * the LDS block of the padded system (SlSolve: its offsets, its carve, its size), the collection of the waves'
//     Gram partials into it (sl_gram_collect), the pivot floor and the L D L^T solve on one wave (sl_ldlt_solve);
//   * the E-step's fixed point on the threads' own samples (sl_estep_fixed_point) and the outer stop test
//     (sl_theta_moved);
//   * the batch forms' limit (SL_MAXBATCH: the estimator kernels as `template <..., bool BATCH>`, workgroup b on
//     problem b of a contiguous batch behind pointer offsets at kernel entry; a slice of a batch is 8-byte aligned,
//     which is what every fp64 load of these kernels -- all of them scalar doubles -- asks).
// Device code and the constants it shares with the host.  The host side of the entries -- the argument checks, the
// launch, the dispatch tables -- is rlvi_sl_launch.h.
// linreg_rlvi_kernel (standard.hip) is held to the instructions it had: it takes the offsets, the pivot floor and
// sl_block_sum2 from here and keeps the Gram collection, the solve, the fixed point and the stop test in place --
// each of them called from here moves its register allocation, and single cells of its sweep by up to 2 % either way
// (profiles/r17_sl_header.md).  Its fit (sl_wls, sl_residuals: that text, verbatim) lives in rlvi_linreg.h, which the
// RRM and Huber regressions (robust_linreg.hip) share; RRM's weight rule is rlvi_rrm.h.
#pragma once
#include "rlvi_common.h"

namespace rlvi {

typedef double sd4_t __attribute__((ext_vector_type(4)));

// (four waves, one per SIMD: a reduction of the fixed point costs every WAVE ~80 instructions whatever it holds, and
//  two waves on a SIMD take turns at its issue slots -- eight waves with two samples per thread measured 0.79 us per
//  inner iteration)
constexpr int SL_THREADS = 256;
constexpr int SL_NW = SL_THREADS / WAVE;
constexpr int SL_DP = 32;                         // the design padded to two 16-column blocks
constexpr int SL_MAXN = 4096;                     // samples the one-workgroup form takes (16 per thread)
constexpr int64_t SL_MAXBATCH = 1 << 20;          // problems of one batch launch (one workgroup each)
constexpr int SL_GPITCH = SL_DP + 1;
constexpr double SL_EPS = 2.220446049250313e-16;

// 1 / x to working precision: v_rcp_f64 + two Newton steps (the factorisation's pivots; not correctly rounded,
// 1e-16 relative, and a tenth of the IEEE division's instruction count on a wave that issues alone)
__device__ __forceinline__ double sl_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return r;
}
// the value is needed HERE, whatever later selects do with it: keeps the compiler from sinking a load into the
// branch of the select that consumes it (a load under a branch is waited for before the next one is issued)
__device__ __forceinline__ void sl_keep(double &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ double sl_readlane(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(b & 0xFFFFFFFFll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// ---- block reductions.  `slots` is [2 parities][SL_NW waves][STRIDE] doubles (sl_slot_doubles(STRIDE)); every
// reduction of a kernel uses the kernel's one STRIDE (its largest K), so one area serves them all.  A reduction is
// wave butterflies, lane 0 of each wave to the slots of the current parity, ONE barrier, everybody combines the waves
// in wave order and flips the parity: the slots of parity p are not written again before everybody has passed the
// NEXT barrier, i.e. has read them.
constexpr int sl_slot_doubles(int stride) { return 2 * SL_NW * stride; }

// v[0 .. K) summed over the workgroup, every thread gets the totals (lane butterfly, then waves 0 .. 3)
template <int K, int STRIDE>
__device__ __forceinline__ void sl_block_sum(double (&v)[K], double *slots, int &parity) {
    static_assert(K <= STRIDE, "slot size");
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    double *s = slots + (size_t)parity * SL_NW * STRIDE;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[wave * STRIDE + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < SL_NW; ++w) t += s[w * STRIDE + k];
        v[k] = t;
    }
    parity ^= 1;
}
// {a, b}: sl_block_sum<2> with a body of its own -- linreg_rlvi_kernel is held to the parent's instructions
// (profiles/r17_sl_header.md: any other spelling moves single cells of its sweep by 1 %)
template <int STRIDE = 2>
__device__ __forceinline__ void sl_block_sum2(double &a, double &b, double *slots, int &parity) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    a = wave_sum(a);
    b = wave_sum(b);
    double *s = slots + (size_t)parity * SL_NW * STRIDE;
    if (lane == 0) { s[STRIDE * wave] = a; s[STRIDE * wave + 1] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
#pragma unroll
    for (int w = 0; w < SL_NW; ++w) { ta += s[STRIDE * w]; tb += s[STRIDE * w + 1]; }
    a = ta; b = tb;
    parity ^= 1;
}

// the largest (MIN: and the smallest) of the threads' values, on every thread
template <bool MIN, int STRIDE>
__device__ __forceinline__ void sl_block_extrema(double &lo, double &hi, double *slots, int &parity) {
    static_assert(STRIDE >= 2, "slot size");
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    double *s = slots + (size_t)parity * SL_NW * STRIDE;
    hi = wave_max(hi);
    if (MIN) lo = wave_min(lo);
    if (lane == 0) {
        s[wave * STRIDE] = hi;
        if (MIN) s[wave * STRIDE + 1] = lo;
    }
    __syncthreads();
    double a = MIN ? s[1] : 0.0, b = s[0];
#pragma unroll
    for (int w = 1; w < SL_NW; ++w) {
        if (MIN) a = s[w * STRIDE + 1] < a ? s[w * STRIDE + 1] : a;
        b = s[w * STRIDE] > b ? s[w * STRIDE] : b;
    }
    lo = a; hi = b;
    parity ^= 1;
}
template <int STRIDE = 2>
__device__ __forceinline__ double sl_block_max(double v, double *slots, int &parity) {
    double none = 0.0;
    sl_block_extrema<false, STRIDE>(none, v, slots, parity);
    return v;
}
template <int STRIDE = 2>
__device__ __forceinline__ void sl_block_minmax(double &lo, double &hi, double *slots, int &parity) {
    sl_block_extrema<true, STRIDE>(lo, hi, slots, parity);
}

// ---- the LDS block of the padded system: what the regressions' kernels carve behind their own per-sample vectors.
// The offsets (in doubles) are the ONE description: the carve and the launchers' sizes both come from them.
struct SlSolve {
    double *red;        // [SL_NW][3][256]  Gram partials of the waves
    double *G;          // [SL_DP][SL_GPITCH]
    double *LT;         // [SL_DP][SL_GPITCH]  L^T of the factorisation (row j = column j of L)
    double *th;         // [SL_DP] the unknowns, [SL_DP] the previous outer iteration's
    double *rhs;        // [SL_DP] column D of the Gram matrix
    double *slots;      // [2][SL_NW][2]
    int *flag;          // [4]
};
enum : int {
    SL_OFF_RED = 0,
    SL_OFF_G = SL_OFF_RED + SL_NW * 3 * 256,
    SL_OFF_LT = SL_OFF_G + SL_DP * SL_GPITCH,
    SL_OFF_TH = SL_OFF_LT + SL_DP * SL_GPITCH,
    SL_OFF_RHS = SL_OFF_TH + 2 * SL_DP,
    SL_OFF_SLOTS = SL_OFF_RHS + SL_DP,
    SL_OFF_FLAG = SL_OFF_SLOTS + sl_slot_doubles(2),
    SL_SOLVE_DOUBLES = SL_OFF_FLAG + 2
};
__device__ __forceinline__ void sl_solve_carve(SlSolve &s, double *base) {
    s.red = base + SL_OFF_RED;
    s.G = base + SL_OFF_G;
    s.LT = base + SL_OFF_LT;
    s.th = base + SL_OFF_TH;
    s.rhs = base + SL_OFF_RHS;
    s.slots = base + SL_OFF_SLOTS;
    s.flag = reinterpret_cast<int *>(base + SL_OFF_FLAG);
}

// The waves' MFMA partials of the Gram matrix (a00; with NB = 2 also a01, a11: the blocks [0][1] and [1][1] of 16 x 16)
// -> s.red, summed in wave order (deterministic) -> s.G: the D x D system PADDED WITH THE IDENTITY to SL_DP rows (a
// padded row has pivot 1 and no coupling: the factorisation is straight-line code without a guard), RIDGE: with the
// identity added inside the D x D block as well; column D, the right-hand side, set aside in s.rhs.  Element e of a
// block = (result r, lane): row (lane >> 4) + 4 r, column lane & 15.  All threads call; ends with a barrier.
template <int NB, bool RIDGE>
__device__ __forceinline__ void sl_gram_collect(const SlSolve &s, int D, sd4_t a00, sd4_t a01, sd4_t a11) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    constexpr int NBLK = NB > 1 ? 3 : 1;
    double *my = s.red + (size_t)wave * 3 * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        my[0 * 256 + r * 64 + lane] = a00[r];
        if (NB > 1) {
            my[1 * 256 + r * 64 + lane] = a01[r];
            my[2 * 256 + r * 64 + lane] = a11[r];
        }
    }
    __syncthreads();
    for (int e = tid; e < NBLK * 256; e += SL_THREADS) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < SL_NW; ++w) sum += s.red[(size_t)w * 3 * 256 + e];
        const int blk = e >> 8, r = (e >> 6) & 3, l = e & 63;
        const int row = (blk == 2 ? 16 : 0) + (l >> 4) + 4 * r, col = (blk >= 1 ? 16 : 0) + (l & 15);
        const double one = row == col ? 1.0 : 0.0;
        // (RIDGE is a compile-time flag, not `sum + 0.0`: that would turn a -0.0 into +0.0)
        const double v = (row < D && col < D) ? (RIDGE ? sum + one : sum) : one;
        s.G[row * SL_GPITCH + col] = v;
        if (blk == 1) s.G[col * SL_GPITCH + row] = v;
        if (col == D && row < D) s.rhs[row] = sum;      // (ONE writer per entry: the mirrored element of a diagonal
                                                        //  block is another rounding of the same sum)
    }
    __syncthreads();
}

// a pivot of a d x d system is "safely positive" above this fraction of a diagonal entry.  Which entry is the
// caller's question: the pivot's OWN (linear regression, standard.hip and wls.hip: pivot / own entry is 1 - R^2 of the
// column on those before it, free of column scale) or the LARGEST (sl_ldlt_solve below, as logistic regression calls
// it -- its ridge bounds every pivot from below and it raises instead of returning a number -- and the covariance of
// moments.hip)
__device__ __forceinline__ double sl_pivot_floor(double dmax, int d) { return dmax * (double)d * 64.0 * SL_EPS; }

// ONE WAVE: G x = rhs by G = L D L^T for the symmetric positive definite G [SL_DP][SL_GPITCH] in LDS, padded with
// the identity beyond its d rows and solved as DS >= d rows -- straight-line code, no guard inside the
// factorisation.  Row t of the lower triangle lives in lane t's registers, pivots and columns travel by
// v_readlane: no LDS round trip and no barrier per pivot.  LT [SL_DP][SL_GPITCH] is scratch (L^T, for the back
// substitution).  x[0 .. d) and *flag (1: a pivot was not safely positive, or not a number) are written; the caller
// puts a workgroup barrier behind the call.
template <int DS>
__device__ __forceinline__ void sl_ldlt_solve(const double *G, double *LT, const double *rhs, int d, double *x,
                                              int *flag) {
    const int lane = threadIdx.x & (WAVE - 1);
    int t = lane & (SL_DP - 1);
    // (opaque: the lane masks t > j, t == j below are loop-invariant across the estimator's outer loop, and
    //  hoisted there they are 2 DP scalar register pairs that spill)
    asm volatile("" : "+v"(t));
    double g[DS];
#pragma unroll
    for (int c = 0; c < DS; ++c) g[c] = G[t * SL_GPITCH + c];
    double b = t < d ? rhs[t < SL_DP ? t : 0] : 0.0;
    double dmax = t < d ? G[t * SL_GPITCH + t] : 0.0;
    dmax = wave_max(dmax);
    const double piv_min = sl_pivot_floor(dmax, d);
    bool bad = !(dmax == dmax);
    double dinv = 0.0;                       // lane j: 1 / D_j
#pragma unroll
    for (int j = 0; j < DS; ++j) {
        const double piv = sl_readlane(g[j], j);
        bad = bad || (j < d && !(piv > piv_min));
        const double inv = sl_rcp(piv);
        const double l = g[j] * inv;                              // L[t][j] for t > j
        dinv = t == j ? inv : dinv;
#pragma unroll
        for (int c = j + 1; c < DS; ++c) {
            const double lc = sl_readlane(g[j], c);              // G[c][j] = L[c][j] D_j
            g[c] = __builtin_fma(-l, lc, g[c]);                  // (lanes t < c compute values nobody reads)
            // (eight broadcasts at a time: all 31 of a pivot hoisted at once do not fit the scalar registers)
            if (((c - j) & 7) == 0) __builtin_amdgcn_sched_barrier(0);
        }
        g[j] = t > j ? l : 0.0;                                   // strictly lower part of L; 0 elsewhere
        LT[j * SL_GPITCH + t] = g[j];                             // row j of L^T: for the back substitution
        __builtin_amdgcn_sched_barrier(0);
    }
    // L z = b (lane t ends with z_t; g[j] = 0 for t <= j: no mask), then z / D
#pragma unroll
    for (int j = 0; j < DS; ++j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
    b *= dinv;
    // L^T x = z: lane t needs column t of L = row t of L^T (0 for c <= t: no mask)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int c = 0; c < DS; ++c) g[c] = LT[t * SL_GPITCH + c];
#pragma unroll
    for (int j = DS - 1; j >= 1; --j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
    if (lane < d) x[lane] = b;
    if (lane == 0) flag[0] = bad ? 1 : 0;
}

// update_weights(losses) (standard-learning/rlvi.py:8-20) on this thread's E samples tid + 256 j: e[j] =
// exp(-losses) (0 for a sample past n), w[j] starts at 0.95 (0 past n) and ends as the new weights.  One block sum
// per iteration; every thread takes the same stop decision.  Returns the iterations taken.
template <int E, int STRIDE = 2>
__device__ __forceinline__ int sl_estep_fixed_point(const double (&e)[E], double (&w)[E], int n, double etol,
                                                    int emaxiter, double *slots, int &parity) {
    const int tid = threadIdx.x;
    const double invn = 1.0 / (double)n;
    double ratio;
    { const double eps = 1.0 - 0.95; ratio = eps / (1.0 - eps); }
    int it = 0;
    while (it < emaxiter) {
        double sse = 0.0, sum = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            // rlvi.py:15.  (A reciprocal + Newton + correction in place of the IEEE division, with a wave-uniform
            // branch for operands near the ends of the exponent range, and the stop test on the squares, were
            // measured: 0.70 us per iteration against 0.57 -- every ballot-and-branch is a scalar round trip on
            // a wave that issues alone.)
            double nw = e[j] / (ratio + e[j]);
            nw = (tid + j * SL_THREADS < n) ? nw : 0.0;
            const double dd = nw - w[j];
            sse = __builtin_fma(dd, dd, sse);
            sum += nw;
            w[j] = nw;
        }
        sl_block_sum2<STRIDE>(sse, sum, slots, parity);
        ++it;
        if (sqrt(sse) < etol) break;                               // rlvi.py:16-19 (assign, then break)
        const double eps = 1.0 - sum * invn;                       // rlvi.py:13-14
        ratio = eps / (1.0 - eps);
    }
    return it;
}

// the outer stop test: false when ||theta - prev|| / ||prev|| <= tol for th[0 .. D) against th[SL_DP .. SL_DP + D)
// (rlvi.py:85-87, :104-106) -- every wave from LDS, the same bits everywhere
__device__ __forceinline__ bool sl_theta_moved(const double *th, int D, double tol) {
    const int lane = threadIdx.x & (WAVE - 1);
    const double tn = lane < D ? th[lane] : 0.0, tp = lane < D ? th[SL_DP + lane] : 0.0;
    const double dn = wave_sum((tn - tp) * (tn - tp)), pn = wave_sum(tp * tp);
    return !(sqrt(dn) / sqrt(pn) <= tol);
}

}  // namespace rlvi
