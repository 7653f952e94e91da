// What the one-workgroup fp64 estimators (standard.hip: linear regression, the online weights; logreg.hip: logistic
// regression) share: the workgroup's shape, the two-value block sum, the reciprocal, the lane broadcast, the
// L D L^T solve of a padded system on one wave and the E-step's fixed point on the threads' own samples.
// (linreg_rlvi_kernel keeps its own copies of the last two in place -- sl_wls's factorisation and the kernel's E-step
//  loop in standard.hip, each marked there: calling them from here moves the register allocation of some of its
//  variants, and tools/isa_same.py holds that kernel to the instructions it had.  A change to either copy belongs in
//  both; moving linreg onto this header is for a change that may alter its instructions and re-measures it.)
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
constexpr int SL_GPITCH = SL_DP + 1;

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

// {a, b} summed over the workgroup, every thread gets the totals: wave butterflies, one slot pair per wave in
// `slots` (two parities x SL_NW x 2 doubles), ONE barrier; the slots of parity p are not written again before
// everybody has passed the NEXT barrier, i.e. has read them.
__device__ __forceinline__ void sl_block_sum2(double &a, double &b, double *slots, int &parity) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    a = wave_sum(a);
    b = wave_sum(b);
    double *s = slots + (size_t)parity * SL_NW * 2;
    if (lane == 0) { s[2 * wave] = a; s[2 * wave + 1] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
#pragma unroll
    for (int w = 0; w < SL_NW; ++w) { ta += s[2 * w]; tb += s[2 * w + 1]; }
    a = ta; b = tb;
    parity ^= 1;
}

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
    const double piv_min = dmax * (double)d * 64.0 * 2.220446049250313e-16;
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
template <int E>
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
            double nw = e[j] / (ratio + e[j]);                     // rlvi.py:15
            nw = (tid + j * SL_THREADS < n) ? nw : 0.0;
            const double dd = nw - w[j];
            sse = __builtin_fma(dd, dd, sse);
            sum += nw;
            w[j] = nw;
        }
        sl_block_sum2(sse, sum, slots, parity);
        ++it;
        if (sqrt(sse) < etol) break;                               // rlvi.py:16-19 (assign, then break)
        const double eps = 1.0 - sum * invn;                       // rlvi.py:13-14
        ratio = eps / (1.0 - eps);
    }
    return it;
}

}  // namespace rlvi
