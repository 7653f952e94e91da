// The two robust linear regressions the reference plots beside RLVI's (standard-learning/main.py:248-357) that are
// iterations around a least-squares solve, as ONE launch each:
//
//   rlvi_rrm_linear_regression_f64     standard-learning/rrm.py:55-73     linear_regression(X, y, eps, maxiter, tol)
//   rlvi_huber_linear_regression_f64   standard-learning/huber.py:13-40   linear_regression(X, y, c, sigma0)
//
// and their batch forms (workgroup b on problem b, the bits of the single launch).  One persistent workgroup of four
// waves with the skeleton, the LDS block and the dispatch table of linreg_rlvi_kernel (standard.hip); the shared
// pieces come from rlvi_linreg.h (sl_wls, sl_residuals, sl_ldlt_factor, sl_ldlt_substitute) and rlvi_rrm.h
// (mo_estep_rrm), one copy of each.
//   * RRM: weights 1 / n, then `maxiter` times {the RRM rule on the squared residuals, a weighted fit, the squared
//     residuals} with the stop test ||theta - prev|| / ||prev|| <= tol after each refit.  The rule's block sums of three
//     values use a slot area of their own behind the solve's block.
//   * Huber: X^T X is formed and factored ONCE (sl_wls with unit weights leaves X^T X, X^T y and the pivot verdict in
//     LDS; sl_ldlt_factor keeps L and 1 / D there); an iteration is the signed residuals, two clips, one block sum for
//     the scale, X^T r_psi on the matrix cores with r_psi as the B operand (one instruction per 4-row panel and column
//     block where the Gram matrix takes three), and one substitution.  The resident form (n <= 1024, d <= 23) reads
//     global memory once.
// Everything read from LDS is written by this workgroup first.  Sums are fp64 in a fixed order: same inputs, same bits.
#include <math.h>

#include "rlvi_linreg.h"
#include "rlvi_rrm.h"
#include "rlvi_sl_launch.h"

namespace rlvi {

constexpr int RL_STRIDE = 3;                              // values of the RRM rule's block sums
constexpr int RL_EXTRA_DOUBLES = SL_DP;                   // behind SlShared's LDS: the rule's slots (24) | Huber's 1 / D (32)
static_assert(sl_slot_doubles(RL_STRIDE) <= RL_EXTRA_DOUBLES, "the rule's slot area");

// SlShared on the kernel's LDS as linreg_rlvi_kernel carves it; returns the RL_EXTRA_DOUBLES behind it
template <int NB, bool RES>
__device__ __forceinline__ double *rl_carve(SlShared &sh, double *sm, int npad) {
#if RLVI_STAMPS
    sh.dbg = nullptr;
    sh.nst = 1 << 30;                                     // (these kernels leave no stamps)
#endif
    sh.wsh = sm;
    sh.rsh = sh.wsh + npad;
    double *const solve = sh.rsh + npad;
    sh.red = solve + SL_OFF_RED;
    sh.G = solve + SL_OFF_G;
    sh.LT = solve + SL_OFF_LT;
    sh.th = solve + SL_OFF_TH;
    sh.rhs = solve + SL_OFF_RHS;
    sh.slots = solve + SL_OFF_SLOTS;
    sh.flag = reinterpret_cast<int *>(solve + SL_OFF_FLAG);
    sh.x1s = solve + SL_SOLVE_DOUBLES;
    return sh.x1s + ((RES && NB > 1) ? 1024 * 8 : 0);
}

// the resident design of sl_wls / sl_residuals (RES): lane (i, kk) of wave w keeps [X | y][4 (w + 4 k) + kk][i], k < 64,
// in xr, columns 16 .. 23 go to sh.x1s; 0 for rows past n and columns past d.  (linreg_rlvi_kernel has these loads in
// its own body: called from a function its register allocation moves -- profiles/r23_robust_linreg.md -- and that
// kernel is held to the instructions it had.)  Then the vectors every fit starts from: wsh = w0 (0 past n), rsh, th, G
// and LT zeroed -- LT as well: a lane beyond the padded system reads rows of it that no factorisation writes.  Ends with
// a barrier.
template <int NB, bool RES>
__device__ __forceinline__ void rl_load_design(const SlShared &sh, const double *__restrict__ X,
                                               const double *__restrict__ y, int n, int d, int npad, double w0,
                                               double (&xr)[RES ? SL_XS : 1]) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if constexpr (RES) {
        const int i = lane & 15, kk = lane >> 4;
        if (i <= d) {                                  // (one branch around all loads: they are in flight together)
#pragma unroll
            for (int k = 0; k < SL_XS; ++k) {
                const int row = 4 * (wave + SL_NW * k) + kk;
                const int rr = row < n ? row : 0;
                xr[k] = *(i < d ? X + (size_t)rr * d + i : y + rr);
            }
        } else {
#pragma unroll
            for (int k = 0; k < SL_XS; ++k) xr[k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < SL_XS; ++k) xr[k] = (4 * (wave + SL_NW * k) + kk < n) ? xr[k] : 0.0;
        if (NB > 1) {
            for (int q0 = tid; q0 < 1024 * 8; q0 += 8 * SL_THREADS) {        // eight loads in flight per thread
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u * SL_THREADS;
                    const int row = q >> 3, col = 16 + (q & 7);
                    const int rr = row < n ? row : 0;
                    v[u] = *(col < d ? X + (size_t)rr * d + col : y + rr);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u * SL_THREADS;
                    const int row = q >> 3, col = 16 + (q & 7);
                    sl_keep(v[u]);
                    sh.x1s[q] = (row < n && col <= d) ? v[u] : 0.0;
                }
            }
        }
    } else {
        xr[0] = 0.0;
    }
    for (int q = tid; q < npad; q += SL_THREADS) {
        sh.wsh[q] = q < n ? w0 : 0.0;
        sh.rsh[q] = 0.0;
    }
    for (int q = tid; q < 2 * SL_DP; q += SL_THREADS) sh.th[q] = 0.0;
    for (int q = tid; q < SL_DP * SL_GPITCH; q += SL_THREADS) {
        sh.G[q] = 0.0;
        sh.LT[q] = 0.0;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------
// rrm.linear_regression (rrm.py:55-73).  info = { outer iterations, evaluations of the last root-find, evaluations in
// all, flag }; flag 1: a pivot was not safely positive (the first fit's, or a later one's: weights that underflow to
// exactly 0 take rows out of the design) -- nothing written, the caller takes the general path; 2: a loss was not
// finite -- nothing written; 3: a root-find hit MO_ROOT_CAP (RLVI_ST_NOCONV in the workspace, the results written).
// ---------------------------------------------------------------------------------------
template <int E, int DS, int NB, bool RES, bool BATCH>
__global__ __launch_bounds__(SL_THREADS) void linreg_rrm_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int n, int d, int npad, int maxiter, double tol,
    double eps, double *__restrict__ theta_out, double *__restrict__ w_out, int32_t *__restrict__ info,
    int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;                   // (64-bit offsets: B n d passes 2^31)
        X += b * (size_t)n * (size_t)d;
        y += b * (size_t)n;
        theta_out += b * (size_t)d;
        w_out += b * (size_t)n;
        info += b * 4;
    }
    SlShared sh;
    double *const slots3 = rl_carve<NB, RES>(sh, sm, npad);
    const int tid = threadIdx.x;
    int parity = 0, parity3 = 0;
    double xr[RES ? SL_XS : 1];
    rl_load_design<NB, RES>(sh, X, y, n, d, npad, 1.0 / (double)n, xr);      // weights = 1 / n (rrm.py:56)

    int outer = 0, evals_last = 0, evals_all = 0, flag = 0;
    bool capped = false;
    // rrm.py:57-59: the first fit and its losses (the squared residuals, no variance: sl_residuals leaves them in rsh)
    if (!sl_wls<DS, NB, RES>(sh, X, y, n, d, xr)) {
        flag = 1;
    } else {
        sl_residuals<NB, RES>(sh, X, y, n, d, parity, xr);
        while (outer < maxiter) {                                    // rrm.py:61
            ++outer;
            double l[E], w[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                l[j] = q < n ? sh.rsh[q] : 0.0;
                w[j] = 0.0;
            }
            bool had_root;
            const int rc = mo_estep_rrm<E, RL_STRIDE>(l, w, n, eps, slots3, parity3, evals_last, had_root);   // :62
            if (rc == 1) { flag = 2; break; }
            capped = capped || rc == 2;
            evals_all += evals_last;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                if (q < n) sh.wsh[q] = w[j];
            }
            if (tid < SL_DP) sh.th[SL_DP + tid] = sh.th[tid];        // prev_theta (rrm.py:64)
            __syncthreads();
            if (!sl_wls<DS, NB, RES>(sh, X, y, n, d, xr)) { flag = 1; break; }      // rrm.py:65-66
            sl_residuals<NB, RES>(sh, X, y, n, d, parity, xr);                      // rrm.py:67
            if (!sl_theta_moved(sh.th, d, tol)) break;                              // rrm.py:69-71
        }
    }
    if (flag == 0) {
        for (int q = tid; q < n; q += SL_THREADS) w_out[q] = sh.wsh[q];
        if (tid < d) theta_out[tid] = sh.th[tid];
    }
    if (tid == 0) {
        info[0] = outer;
        info[1] = evals_last;
        info[2] = evals_all;
        info[3] = flag != 0 ? flag : (capped ? 3 : 0);
        if (flag == 0 && capped) atomicOr(status, RLVI_ST_NOCONV);
    }
}

// ---------------------------------------------------------------------------------------
// Huber's pieces
// ---------------------------------------------------------------------------------------
// sigma psi(r / sigma, c) (huber.py:5-10 at :23, :27) as a clip of r at cs = c sigma
__device__ __forceinline__ double rl_clip(double r, double cs) { return fabs(r) <= cs ? r : __builtin_copysign(cs, r); }

// r_i = y_i - x_i.theta (theta = sh.th[0 .. d)) -> sh.rsh[i], i < n (the entries past n stay 0).  Ends with a barrier.
template <int NB, bool RES>
__device__ __forceinline__ void rl_signed_residuals(const SlShared &sh, const double *__restrict__ X,
                                                    const double *__restrict__ y, int n, int d,
                                                    const double (&xr)[RES ? SL_XS : 1]) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    if constexpr (RES) {
        // from the resident panels, as sl_residuals: with c = [theta; -1 in column d] a row's x.theta - y is the sum
        // over the 16 lanes of its group (a four-step butterfly per panel)
        const double c0 = i < d ? sh.th[i] : (i == d ? -1.0 : 0.0);
        const int j1 = 16 + (i & 7);
        const double c1 = (NB > 1 && i < 8) ? (j1 < d ? sh.th[j1 < SL_DP ? j1 : 0] : (j1 == d ? -1.0 : 0.0)) : 0.0;
#pragma unroll
        for (int k0 = 0; k0 < SL_XS; k0 += 8) {
            if (4 * (wave + SL_NW * k0) < n) {                        // (wave-uniform: a short design skips its empty blocks)
                double p[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;      // < 1024 = the padded length of rsh / x1s
                    p[u] = xr[k0 + u] * c0;
                    if (NB > 1) p[u] = __builtin_fma(sh.x1s[row * 8 + (i & 7)], c1, p[u]);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;
                    const double s = group_allreduce<16>(p[u], FAdd());
                    if (i == 0 && row < n) sh.rsh[row] = -s;
                }
            }
        }
    } else {
        // X[16 rb .. +15] . theta on the matrix cores: SL_RU row blocks per wave and trip.  The loads, the
        // sched_barrier and the masks are those of sl_residuals' streamed branch (rlvi_linreg.h), which must stay as it is
        // for linreg_rlvi_kernel: A CHANGE TO THAT LOAD PATTERN HAS TO BE MADE IN BOTH PLACES.
        const int blocks = (n + 15) / 16;
        double bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = 4 * u + kk;
            const double tv = sh.th[k < d ? k : 0];
            bv[u] = k < d ? tv : 0.0;
        }
        for (int rb0 = wave; rb0 < blocks; rb0 += SL_RU * SL_NW) {
            double a[SL_RU][8], yv[SL_RU];
#pragma unroll
            for (int q = 0; q < SL_RU; ++q) {
                const int rb = rb0 + q * SL_NW;
                const int row = 16 * rb + i;
                const double *xrow = X + (size_t)(row < n ? row : 0) * d;
#pragma unroll
                for (int u = 0; u < 8; ++u) a[q][u] = xrow[(4 * u + kk) < d ? 4 * u + kk : 0];      // (branch-free)
                const int r = 16 * rb + kk + 4 * (i & 3);
                yv[q] = y[r < n ? r : 0];
            }
            __builtin_amdgcn_sched_barrier(0);        // every load of the trip is out before the first value is used
#pragma unroll
            for (int q = 0; q < SL_RU; ++q) {
                const int rb = rb0 + q * SL_NW;
                const bool rok = 16 * rb + i < n;
                sd4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    sl_keep(a[q][u]);
                    const double av = (rok && 4 * u + kk < d) ? a[q][u] : 0.0;
                    if (4 * u < d) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], acc, 0, 0, 0);
                }
                sl_keep(yv[q]);
                const int r = 16 * rb + kk + 4 * i;                  // lane (i < 4, kk) holds rows kk + 4 r' in acc[r']
                if (i < 4 && r < n) {
                    const double p = i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3];
                    sh.rsh[r] = yv[q] - p;
                }
            }
        }
    }
    __syncthreads();
}

// The waves' partials of X^T v, v = sh.rsh (0 past n) -> sh.red[wave][32]; ends with a barrier.  The Gram loop of
// sl_wls with v in the place of the second factor: every column of the B operand is v, so every column of the 16 x 16
// result is X_blk^T v and lane (0, kk) reads entries kk + 4 r of it.  (Entry d, where the block holds y, is y.v: unused.)
template <int NB, bool RES>
__device__ __forceinline__ void rl_xt_v(const SlShared &sh, const double *__restrict__ X, int n, int d,
                                        const double (&xr)[RES ? SL_XS : 1]) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    sd4_t a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0;
    if constexpr (RES) {
#pragma unroll
        for (int k0 = 0; k0 < SL_XS; k0 += 8) {
            if (4 * (wave + SL_NW * k0) < n) {
                double v[8], x1[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;
                    v[u] = sh.rsh[row];
                    x1[u] = (NB > 1 && i < 8) ? sh.x1s[row * 8 + (i & 7)] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[k0 + u], v[u], a0, 0, 0, 0);
                    if (NB > 1) a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], v[u], a1, 0, 0, 0);
                }
            }
        }
    } else {
        // (the streamed Gram loop of sl_wls -- rlvi_linreg.h -- with v as the second factor; that loop must stay as it is
        //  for linreg_rlvi_kernel: A CHANGE TO ITS LOAD PATTERN HAS TO BE MADE IN BOTH PLACES)
        const int steps = (n + 3) / 4;
        for (int s0 = wave; s0 < steps; s0 += SL_GU * SL_NW) {
            double x0[SL_GU], x1[SL_GU], v[SL_GU];
            int rr[SL_GU];
#pragma unroll
            for (int u = 0; u < SL_GU; ++u) {
                const int s = s0 + u * SL_NW;
                const int row = 4 * s + kk;
                const bool ok = s < steps && row < n;
                rr[u] = ok ? row : 0;
                v[u] = sh.rsh[rr[u]];
                x0[u] = 0.0;
                x1[u] = 0.0;
            }
            if (i < d) {                               // (one branch around all loads of a block: in flight together)
#pragma unroll
                for (int u = 0; u < SL_GU; ++u) x0[u] = X[(size_t)rr[u] * d + i];
            }
            if (NB > 1 && 16 + i < d) {
#pragma unroll
                for (int u = 0; u < SL_GU; ++u) x1[u] = X[(size_t)rr[u] * d + 16 + i];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < SL_GU; ++u) {
                const int s = s0 + u * SL_NW;
                const bool ok = s < steps && 4 * s + kk < n;
                sl_keep(x0[u]);
                if (NB > 1) sl_keep(x1[u]);
                v[u] = ok ? v[u] : 0.0;
                a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ok ? x0[u] : 0.0, v[u], a0, 0, 0, 0);
                if (NB > 1) a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ok ? x1[u] : 0.0, v[u], a1, 0, 0, 0);
            }
        }
    }
    if (i == 0) {
        double *my = sh.red + wave * SL_DP;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            my[kk + 4 * r] = a0[r];
            my[16 + kk + 4 * r] = NB > 1 ? a1[r] : 0.0;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------
// huber.linear_regression (huber.py:13-40), the reference's `while True` capped at maxiter.  info = { iterations, 0,
// 0, flag }; flag 1: X^T X has a pivot that is not safely positive -- nothing written; 2: a scale that is not positive
// and finite (an exact fit: sigma = 0) or a theta that is not finite -- nothing written; 3: the iteration still moved
// when the cap was reached (RLVI_ST_NOCONV in the workspace, the last iterate written).  maxiter = 0: theta0 and sigma0.
// ---------------------------------------------------------------------------------------
template <int E, int DS, int NB, bool RES, bool BATCH>
__global__ __launch_bounds__(SL_THREADS) void linreg_huber_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int n, int d, int npad, int maxiter, double c,
    double sigma0, double alpha, double *__restrict__ theta_out, double *__restrict__ scale_out,
    int32_t *__restrict__ info, int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;
        X += b * (size_t)n * (size_t)d;
        y += b * (size_t)n;
        theta_out += b * (size_t)d;
        scale_out += b;
        info += b * 4;
    }
    SlShared sh;
    double *const dinv = rl_carve<NB, RES>(sh, sm, npad);
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int parity = 0;
    double xr[RES ? SL_XS : 1];
    rl_load_design<NB, RES>(sh, X, y, n, d, npad, 1.0, xr);

    int it = 0, flag = 0;
    double s0 = sigma0, sigma = sigma0;
    double t0 = 0.0;                                                 // lane t < d of every wave: theta0[t]
    // X^T X, X^T y (sh.G, sh.rhs) and the pivot verdict from the unit-weight fit; then the factorisation that stays
    // (huber.py:17 with the factors kept), theta0 from the first substitution
    if (!sl_wls<DS, NB, RES>(sh, X, y, n, d, xr)) {
        flag = 1;
    } else {
        if (wave == 0) {
            sl_ldlt_factor<DS>(sh.G, sh.LT, d, dinv, sh.flag + 1);
            sl_ldlt_substitute<DS>(sh.LT, dinv, sh.rhs, d, sh.th);
        }
        __syncthreads();
        t0 = lane < d ? sh.th[lane] : 0.0;
        if (sh.flag[1] != 0) flag = 1;
        else if (__any(!(fabs(t0) < __builtin_inf()))) flag = 2;
    }
    const double tna = 2.0 * (double)n * alpha;                      // huber.py:25
    while (flag == 0 && it < maxiter) {
        ++it;
        rl_signed_residuals<NB, RES>(sh, X, y, n, d, xr);            // huber.py:21
        double r[E], ss = 0.0, none = 0.0;
        const double cs0 = c * s0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            r[j] = q < n ? sh.rsh[q] : 0.0;
            const double p = rl_clip(r[j], cs0);                     // huber.py:23
            ss = __builtin_fma(p, p, ss);
        }
        sl_block_sum2(ss, none, sh.slots, parity);
        sigma = sqrt(ss / tna);                                      // huber.py:25
        if (!(sigma > 0.0 && sigma < __builtin_inf())) { flag = 2; break; }
        const double cs = c * sigma;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) sh.rsh[q] = rl_clip(r[j], cs);                // huber.py:27
        }
        __syncthreads();
        rl_xt_v<NB, RES>(sh, X, n, d, xr);                           // X^T r_psi (huber.py:29-30)
        if (wave == 0) {
            if (lane < SL_DP) {
                double s = 0.0;
                if (lane < d) {
#pragma unroll
                    for (int w = 0; w < SL_NW; ++w) s += sh.red[w * SL_DP + lane];      // (wave order)
                }
                sh.rhs[lane] = s;
            }
            sl_ldlt_substitute<DS>(sh.LT, dinv, sh.rhs, d, sh.th + SL_DP);              // delta
        }
        __syncthreads();
        const double dl = lane < d ? sh.th[SL_DP + lane] : 0.0;
        const double tn = t0 + dl, df = tn - t0;                     // huber.py:32
        if (__any(!(fabs(tn) < __builtin_inf()))) { flag = 2; break; }
        const double dn = wave_sum(df * df), pn = wave_sum(t0 * t0);
        const bool moved = sqrt(dn) / sqrt(pn) > 1e-6;               // huber.py:34 (a NaN ends the loop)
        t0 = tn;
        if (!moved) break;
        s0 = sigma;                                                  // huber.py:35-36
        if (tid < d) sh.th[tid] = tn;
        __syncthreads();
        if (it == maxiter) flag = 3;
    }
    if (flag == 0 || flag == 3) {
        if (tid < d) theta_out[tid] = t0;
        if (tid == 0) scale_out[0] = sigma;
    }
    if (tid == 0) {
        info[0] = it;
        info[1] = 0;
        info[2] = 0;
        info[3] = flag;
        if (flag == 3) atomicOr(status, RLVI_ST_NOCONV);
    }
}

// Both forms of both estimators: one workgroup, or (BATCH) one per problem of the batch.  The contract is
// rlvi_linear_regression_f64's with the estimator's own parameters (params_ok) and its second output (out2: RRM's
// weights, Huber's scale); the table and the shape are standard.hip's (sl_linreg_form, sl_linreg_shape), with the rule's
// slots or Huber's 1 / D behind SlShared's LDS.
static int rl_args(const double *X, const double *y, int64_t batch, int64_t n, int64_t d, int maxiter, bool params_ok,
                   double *theta, double *out2, int32_t *info, void *ws) {
    return sl_check_args({X, y, theta, out2, info, ws}, batch, n, d, maxiter >= 0 && params_ok,
                         n <= SL_MAXN && d < SL_DP, {X, y, theta, out2}, {info}, ws);
}

template <bool BATCH>
static int rl_rrm_entry(const double *X, const double *y, int64_t batch, int64_t n, int64_t d, double eps,
                        int maxiter, double tol, double *theta, double *weights, int32_t *info, void *ws,
                        void *stream) {
    if (const int e = rl_args(X, y, batch, n, d, maxiter, rl_eps_ok(eps, n), theta, weights, info, ws)) return e;
    const SlLinregShape s = sl_linreg_shape(n, d, RL_EXTRA_DOUBLES);
    return sl_linreg_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(linreg_rrm_kernel<F::E, F::DS, F::NB, F::RES, BATCH>, batch, s.lds,
                         static_cast<hipStream_t>(stream), X, y, (int)n, (int)d, s.npad, maxiter, tol, eps, theta, weights,
                         info, sl_status(ws));
    });
}

template <bool BATCH>
static int rl_huber_entry(const double *X, const double *y, int64_t batch, int64_t n, int64_t d, double c,
                          double sigma0, int maxiter, double *theta, double *scale, int32_t *info, void *ws,
                          void *stream) {
    if (const int e = rl_args(X, y, batch, n, d, maxiter, c > 0.0 && sigma0 > 0.0, theta, scale, info, ws)) return e;
    const SlLinregShape s = sl_linreg_shape(n, d, RL_EXTRA_DOUBLES);
    const double alpha = rlvi_huber_alpha(c);
    return sl_linreg_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(linreg_huber_kernel<F::E, F::DS, F::NB, F::RES, BATCH>, batch, s.lds,
                         static_cast<hipStream_t>(stream), X, y, (int)n, (int)d, s.npad, maxiter, c, sigma0, alpha, theta,
                         scale, info, sl_status(ws));
    });
}

}  // namespace rlvi

using namespace rlvi;

// alpha = c^2 (1 - F1(c^2)) + F3(c^2) (huber.py:15), F_k the chi-square distribution function with k degrees of freedom:
// F1(c^2) = erf(c / sqrt 2), F3(c^2) = F1(c^2) - sqrt(2 / pi) c exp(-c^2 / 2)
extern "C" double rlvi_huber_alpha(double c) {
    const double f1 = erf(c * 0.70710678118654752440);
    const double f3 = f1 - 0.79788456080286535588 * c * exp(-0.5 * c * c);
    return c * c * (1.0 - f1) + f3;
}

extern "C" int rlvi_rrm_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double eps,
                                              int maxiter, double tol, double *theta, double *weights, int32_t *info,
                                              void *ws, void *stream) {
    return rl_rrm_entry<false>(X, y, 1, n, d, eps, maxiter, tol, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n,
                                                    int64_t d, double eps, int maxiter, double tol, double *theta,
                                                    double *weights, int32_t *info, void *ws, void *stream) {
    return rl_rrm_entry<true>(X, y, batch, n, d, eps, maxiter, tol, theta, weights, info, ws, stream);
}

extern "C" int rlvi_huber_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double c,
                                                double sigma0, int maxiter, double *theta, double *scale, int32_t *info,
                                                void *ws, void *stream) {
    return rl_huber_entry<false>(X, y, 1, n, d, c, sigma0, maxiter, theta, scale, info, ws, stream);
}

extern "C" int rlvi_huber_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n,
                                                      int64_t d, double c, double sigma0, int maxiter, double *theta,
                                                      double *scale, int32_t *info, void *ws, void *stream) {
    return rl_huber_entry<true>(X, y, batch, n, d, c, sigma0, maxiter, theta, scale, info, ws, stream);
}
