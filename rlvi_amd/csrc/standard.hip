// The standard-learning / online-learning estimators as ONE launch each.
//
//   rlvi_linear_regression_f64      standard-learning/rlvi.py:68-89   linear_regression(X, y, maxiter, tol)
//   rlvi_sample_weight_online_f64   online-learning/main.py:293-297   log_proba -> residuals -> update_weights_rlvi
//
// The reference alternates a closed-form E-step (update_weights, rlvi.py:8-20: up to 100 population-wide
// reductions) with a weighted least-squares fit (scipy lstsq on diag(sqrt(w))-scaled rows, rlvi.py:79-80) until
// theta stops moving (rlvi.py:85-87) -- at n = 1000, d = 20 three outer iterations, 135 inner ones and four
// solves of a 20 x 20 system: 40 kflop per product, nothing a launch per step or a host decision per outer
// iteration could ever amortise (round 3: six launches + three torch ops + one host sync per outer iteration,
// 0.62 ms per call).  Here the whole estimator is one persistent workgroup of four waves (one per SIMD):
//   * the samples live in registers (n <= 4096: up to sixteen per thread) and in two LDS vectors (weights, squared
//     residuals); every reduction of the fixed point is a wave butterfly + ONE workgroup barrier (partials in
//     parity-buffered LDS slots, summed in wave order by everybody: all threads take the same stop decision);
//   * the weighted Gram matrix [X | y]^T W [X | y] -- THE dense contraction of the path -- runs on the fp64 matrix
//     cores (v_mfma_f64_16x16x4_f64), sixteen 4-row k-panels of [X | y] per wave and trip with all their loads in
//     flight together (the design stays in the L2); X.theta likewise (16 rows per wave and instruction, k over
//     the columns);
//   * the (d+1) x (d+1) system is factored (L D L^T) and solved by wave 0 with a row per lane in registers and
//     v_readlane broadcasts -- no LDS round trip and no barrier per pivot;
//   * the stop test ||theta - prev|| / ||prev|| <= tol is evaluated by every wave from LDS: no host in the loop,
//     ONE launch, and the host waits once for theta.
// A pivot that says "rank-deficient" (the reference's lstsq then returns the minimum-norm solution) ends the
// launch with info[3] = 1: the caller runs the general path (wls.hip: Jacobi pseudo-inverse) instead.
// Sums are fp64 in a fixed order: same inputs, same bits.
#include <string.h>

#include "rlvi_linreg.h"
#include "rlvi_sl_launch.h"

namespace rlvi {


// BATCH: workgroup b works on problem b of a contiguous batch (X [B, n, d], y [B, n], theta [B, d], weights [B, n],
// info [B, 4]) -- the same code behind wave-uniform pointer offsets, so a problem gets the bits of the single launch;
// a template flag, not arithmetic on blockIdx.x in the one kernel: the single form keeps its instructions
// (profiles/r18_batch.md).  Everything read from LDS is written by this workgroup first (wsh, th, G below; rsh, red,
// rhs, LT, the slots and flag before their first read): a CU's previous workgroup leaves nothing behind that counts.
template <int E, int DS, int NB, bool RES, bool BATCH = false>
__global__ __launch_bounds__(SL_THREADS) void linreg_rlvi_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int n, int d, int npad, int maxiter, double tol,
    double etol, int emaxiter, double *__restrict__ theta_out, double *__restrict__ w_out,
    int32_t *__restrict__ info, unsigned long long *__restrict__ dbg) {
    extern __shared__ double sm[];
    SlShared sh;
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;                   // (64-bit offsets: B n d passes 2^31)
        X += b * (size_t)n * (size_t)d;
        y += b * (size_t)n;
        theta_out += b * (size_t)d;
        w_out += b * (size_t)n;
        info += b * 4;
    }
#if RLVI_STAMPS
    sh.dbg = dbg;
    sh.nst = (BATCH && blockIdx.x != 0) ? (1 << 30) : 0;      // only workgroup 0 leaves stamps
#else
    (void)dbg;
#endif
    sh.wsh = sm;
    sh.rsh = sh.wsh + npad;
    // (the solve's block from rlvi_sl.h's offset table, spelled out: sl_solve_carve on a base struct moves this
    //  kernel's register allocation)
    double *const solve = sh.rsh + npad;
    sh.red = solve + SL_OFF_RED;
    sh.G = solve + SL_OFF_G;
    sh.LT = solve + SL_OFF_LT;
    sh.th = solve + SL_OFF_TH;
    sh.rhs = solve + SL_OFF_RHS;
    sh.slots = solve + SL_OFF_SLOTS;
    sh.flag = reinterpret_cast<int *>(solve + SL_OFF_FLAG);
    sh.x1s = solve + SL_SOLVE_DOUBLES;                  // (= sm + sl_lds_doubles(npad, false))
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    int parity = 0;

    // resident design: the k-panels of column block 0 into registers, columns 16 .. 23 into LDS -- once
    double xr[RES ? SL_XS : 1];
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
    for (int q = tid; q < npad; q += SL_THREADS) sh.wsh[q] = q < n ? 1.0 : 0.0;     // weights = ones (rlvi.py:69)
    for (int q = tid; q < 2 * SL_DP; q += SL_THREADS) sh.th[q] = 0.0;
    for (int q = tid; q < SL_DP * SL_GPITCH; q += SL_THREADS) sh.G[q] = 0.0;
    __syncthreads();

    int outer = 0, inner_last = 0, inner_all = 0;
    bool ok = true;
    const double invn = 1.0 / (double)n;
    for (;;) {
        SL_STAMP();   // outer iteration starts
        // theta from the current weights (rlvi.py:70-71 the first time, :79-80 afterwards), then the residuals
        // and sigma2 (:72-73, :81-82)
        ok = sl_wls<DS, NB, RES>(sh, X, y, n, d, xr);
        if (!ok) break;
        const double sigma2 = sl_residuals<NB, RES>(sh, X, y, n, d, parity, xr);
        if (outer > 0) {
            // ||theta - prev|| / ||prev|| <= tol (rlvi.py:85-87): every wave from LDS, the same bits everywhere
            const double tn = lane < d ? sh.th[lane] : 0.0, tp = lane < d ? sh.th[SL_DP + lane] : 0.0;
            const double dn = wave_sum((tn - tp) * (tn - tp)), pn = wave_sum(tp * tp);
            if (sqrt(dn) / sqrt(pn) <= tol) break;
        }
        if (outer >= maxiter) break;
        ++outer;
        // ---- update_weights(losses) (rlvi.py:8-20, called at :77) on this thread's samples tid + 256 j
        double e[E], w[E];
        const double hs = 0.5 / sigma2;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            const bool v = q < n;
            e[j] = v ? exp(-(sh.rsh[v ? q : 0] * hs)) : 0.0;      // losses = 0.5 r / sigma2 (rlvi.py:74); exp(-losses)
            w[j] = v ? 0.95 : 0.0;                                 // rlvi.py:10
        }
        // (sl_estep_fixed_point<E> of rlvi_sl.h in place, for the same reason as the factorisation in sl_wls)
        double ratio;
        { const double eps = 1.0 - 0.95; ratio = eps / (1.0 - eps); }
        int it = 0;
        SL_STAMP();   // exp done
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
            sl_block_sum2(sse, sum, sh.slots, parity);
            ++it;
            if (sqrt(sse) < etol) break;                           // rlvi.py:16-19 (assign, then break)
            const double eps = 1.0 - sum * invn;                   // rlvi.py:13-14
            ratio = eps / (1.0 - eps);
        }
        SL_STAMP();   // E-step done
        inner_last = it;
        inner_all += it;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) sh.wsh[q] = w[j];
        }
        if (tid < SL_DP) sh.th[SL_DP + tid] = sh.th[tid];          // theta_prev (rlvi.py:78)
        __syncthreads();
    }
    if (ok) {
        for (int q = tid; q < n; q += SL_THREADS) w_out[q] = sh.wsh[q];
        if (tid < d) theta_out[tid] = sh.th[tid];
    }
    if (tid == 0) {
        info[0] = outer;
        info[1] = inner_last;
        info[2] = inner_all;
        info[3] = ok ? 0 : 1;          // 1: rank-deficient (or not finite) -- the caller takes the general path
    }
}

// ---------------------------------------------------------------------------------------
// One mini-batch of the online path: log_proba = log sigmoid(X w + b) (first batch: log 0.5), residuals =
// -log_proba (main.py:293-296 with :84-85), sample_weight = update_weights_rlvi(residuals) (main.py:45-58, :297).
// ---------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(SL_THREADS) void online_weight_kernel(
    const double *__restrict__ X, const double *__restrict__ wv, double b, int first, int n, int d, double tol,
    int maxiter, double *__restrict__ losses_out, double *__restrict__ out, int32_t *__restrict__ out_iters) {
    __shared__ double lsh[SL_MAXN];
    __shared__ double slots[sl_slot_doubles(2)];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    int parity = 0;
    if (first) {
        for (int q = tid; q < n; q += SL_THREADS) lsh[q] = 0.6931471805599453;      // -log(0.5) (main.py:293)
    } else {
        const int blocks = (n + 15) / 16;
        for (int rb = wave; rb < blocks; rb += SL_NW) {
            const int row = 16 * rb + i;
            const bool rok = row < n;
            const double *xrow = X + (size_t)(rok ? row : 0) * d;
            sd4_t acc = {0.0, 0.0, 0.0, 0.0};
            int k0 = 0;
            for (; k0 + 32 <= d; k0 += 32) {                         // eight k-panels per trip, loads in flight together
                double a[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int k = k0 + 4 * u + kk;
                    a[u] = xrow[k];                                 // (row 0 for rows past n: valid, selected away)
                    bv[u] = wv[k];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) { sl_keep(a[u]); a[u] = rok ? a[u] : 0.0; }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bv[u], acc, 0, 0, 0);
            }
            {
                double a[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int k = k0 + 4 * u + kk;
                    a[u] = xrow[k < d ? k : 0];                     // (branch-free loads, selected below)
                    bv[u] = wv[k < d ? k : 0];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int k = k0 + 4 * u + kk;
                    sl_keep(a[u]);
                    sl_keep(bv[u]);
                    a[u] = (rok && k < d) ? a[u] : 0.0;
                    bv[u] = k < d ? bv[u] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (k0 + 4 * u < d) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bv[u], acc, 0, 0, 0);
            }
            if (i < 4) {
                const int r = 16 * rb + kk + 4 * i;
                if (r < n) {
                    const double p = (i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3]) + b;
                    lsh[r] = p >= 0.0 ? log1p(exp(-p)) : -p + log1p(exp(p));      // -log sigmoid(p)
                }
            }
        }
    }
    __syncthreads();
    double e[E], w[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        const bool v = q < n;
        const double l = lsh[v ? q : 0];
        if (v && losses_out != nullptr) losses_out[q] = l;
        e[j] = v ? exp(-l) : 0.0;                                   // main.py:47
        w[j] = v ? 0.5 : 0.0;                                       // main.py:48
    }
    double ratio = 0.5 / (1.0 - 0.5);
    const double invn = 1.0 / (double)n;
    int it = 0;
    while (it < maxiter) {
        double sse = 0.0, sum = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const double t = ratio * e[j];                          // main.py:52 (a sample past n: e = 0, update 0)
            const double nw = t / (1.0 + t);
            const double dd = nw - w[j];
            sse = __builtin_fma(dd, dd, sse);
            sum += nw;
            w[j] = nw;
        }
        sl_block_sum2(sse, sum, slots, parity);
        ++it;
        if (sqrt(sse) < tol) break;                                 // main.py:53-56 (`new` is what is returned either way)
        const double avg = sum * invn;                              // main.py:50-51
        ratio = avg / (1.0 - avg);
    }
    // new /= max(new) * len(new) (main.py:57)
    double mx = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < E; ++j)
        if (tid + j * SL_THREADS < n) mx = w[j] > mx ? w[j] : mx;
    mx = sl_block_max(mx, slots, parity);
    const double den = mx * (double)n;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        if (q < n) out[q] = w[j] / den;
    }
    if (tid == 0 && out_iters != nullptr) *out_iters = it;
}

}  // namespace rlvi

using namespace rlvi;

// 0 when rlvi_linear_regression_f64 takes this shape in its one-launch form (else RLVI_E_LIMIT: the caller
// composes rlvi_wls_solve_f64 / rlvi_linreg_losses_f64 / rlvi_update_weights_f64 itself)
extern "C" int rlvi_linear_regression_check(int64_t n, int64_t d) {
    if (n <= 0 || d <= 0) return RLVI_E_SHAPE;
    return (n <= SL_MAXN && d < SL_DP) ? 0 : RLVI_E_LIMIT;
}

// both forms of the entry: one workgroup, or (BATCH) one per problem -- the single form is the batch form with batch = 1
template <bool BATCH>
static int sl_linreg_entry(const double *X, const double *y, int64_t batch, int64_t n, int64_t d, int maxiter,
                           double tol, double estep_tol, int estep_maxiter, double *theta, double *weights,
                           int32_t *info, void *ws, void *stream) {
    if (const int e = sl_check_args({X, y, theta, weights, info, ws}, batch, n, d, maxiter >= 0 && estep_maxiter >= 0,
                                    n <= SL_MAXN && d < SL_DP, {X, y, theta, weights}, {info}, ws))
        return e;
    const SlLinregShape s = sl_linreg_shape(n, d, 0);
    return sl_linreg_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(linreg_rlvi_kernel<F::E, F::DS, F::NB, F::RES, BATCH>, batch, s.lds,
                         static_cast<hipStream_t>(stream), X, y, (int)n, (int)d, s.npad, maxiter, tol, estep_tol,
                         estep_maxiter, theta, weights, info, stamp_base(ws));
    });
}

extern "C" int rlvi_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, int maxiter,
                                          double tol, double estep_tol, int estep_maxiter, double *theta,
                                          double *weights, int32_t *info, void *ws, void *stream) {
    return sl_linreg_entry<false>(X, y, 1, n, d, maxiter, tol, estep_tol, estep_maxiter, theta, weights, info, ws,
                                  stream);
}

extern "C" int rlvi_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                                int maxiter, double tol, double estep_tol, int estep_maxiter,
                                                double *theta, double *weights, int32_t *info, void *ws,
                                                void *stream) {
    return sl_linreg_entry<true>(X, y, batch, n, d, maxiter, tol, estep_tol, estep_maxiter, theta, weights, info, ws,
                                 stream);
}

extern "C" int rlvi_sample_weight_online_f64(const double *X, const double *w, double b, int first, int64_t n,
                                             int64_t d, double tol, int maxiter, double *losses_out,
                                             double *sample_weight, int32_t *out_iters, void *stream) {
    if (const int e = sl_check_args({sample_weight, sl_when(!first, X), sl_when(!first, w)}, 1, n, d, maxiter >= 0,
                                    n <= SL_MAXN, {X, w, sample_weight, losses_out}))
        return e;
    // (static LDS: no request for more)
    return sl_per_thread<1, 2, 4, 8, 16>(n, [&](auto f) {
        return sl_launch_plain(online_weight_kernel<decltype(f)::E>, 1, 0, static_cast<hipStream_t>(stream), X, w, b,
                               first, (int)n, (int)d, tol, maxiter, losses_out, sample_weight, out_iters);
    });
}
