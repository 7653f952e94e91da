// RLVI's logistic regression as ONE launch (the other half of "the dense X.w contraction in the standard-learning
// linear/logistic path"):
//
//   rlvi_logistic_regression_f64    standard-learning/rlvi.py:92-108   logistic_regression(X, y, maxiter, tol)
//   rlvi_logistic_fit_f64           standard-learning/utils.py:61-73   sklearn_log_reg(X, y, weights): one M-step
//
// The reference alternates the closed-form E-step (update_weights, rlvi.py:8-20) with a liblinear fit (utils.py:
// 66-69: C = 1e2, L2, primal, the bias regularised, the weights divided by their maximum) on 100 .. 200 x 2 designs,
// 2 .. 50 times: latency a launch, a copy or a third-party call per statement can never amortise.  liblinear
// minimises the strictly convex
//     f(v) = 1/2 v.v + C sum_i what_i log(1 + exp(-s_i z_i)),   v = (coef, bias), z = X coef + bias, s = 2 y - 1,
// to its own tol = 1e-4; its Hessian is >= I, the minimiser unique.  Here a damped Newton iteration runs to the
// rounding floor, so the result is the point liblinear approximates: the CONTRACT is the minimiser, not liblinear's
// iterate (DESIGN, "Logistic regression in one launch").
//
// One persistent workgroup of four waves, as linreg_rlvi_kernel (standard.hip):
//   * per sample: z, the Hessian's and the gradient's coefficient in three LDS vectors; s C what and the weight in
//     the registers of the thread that owns the sample (tid + 256 j);
//   * a Newton step is ONE pass for p = sigma(-s z), f and the coefficients (a block sum: one barrier), ONE pass
//     over the design for the Hessian I + Z^T diag(C what p (1 - p)) Z AND the gradient's Z^T (C what s p) -- a
//     weighted Gram matrix of [X | 1] with the gradient's coefficient as one more column of the right factor, on
//     v_mfma_f64_16x16x4_f64 --, the L D L^T solve on wave 0 (rlvi_sl.h), ONE pass Z.delta on the matrix cores, and
//     the Armijo halving on z - t Z.delta: every trial step is the samples' arithmetic + one block sum, nothing is
//     read from memory;
//   * every decision (Newton stop, Armijo, E-step stop, outer stop) is taken by every thread from the same LDS totals:
//     no host in the loop, one launch, the host waits once.
// Every fit starts from v = 0: a fit is then a function of (X, y, weights) alone -- rlvi_logistic_fit_f64 and the
// fits inside the estimator run the same arithmetic, and ||g(0)||, the scale of the stop test, is the first step's
// gradient.  Sums are fp64 in a fixed order: same inputs, same bits.
// The fit itself (lg_fit and its passes, LgShared, the constants) lives in rlvi_logreg.h, which RRM's logistic
// regression (robust_logreg.hip) shares.
#include "rlvi_logreg.h"
#include "rlvi_sl_launch.h"

namespace rlvi {

// mode 0: the estimator (rlvi.py:92-108) -> theta [d + 1] = (intercept, coef), weights [n], losses (may be NULL);
// mode 1: one fit with the caller's weights w_in (utils.py:61-73) -> theta, losses [n].
// BATCH (mode 0 only): workgroup b works on problem b of a contiguous batch (X [B, n, d], y [B, n], theta [B, d + 1],
// weights [B, n], losses [B, n] or NULL, info [B, 4]) behind wave-uniform pointer offsets -- a template flag, as in
// linreg_rlvi_kernel: the single form keeps its instructions.  `status` is the ONE word of the workspace for all
// workgroups (atomicOr); a problem's own flag is info[4 b + 3].  Everything read from LDS is written by this
// workgroup first (th and G here, th and zsh again by every fit, hsh / csh / gv / dl / rhs before their reads).
template <int E, int DS, int NB, bool BATCH = false>
__global__ __launch_bounds__(SL_THREADS) void logreg_rlvi_kernel(
    const double *__restrict__ X, const double *__restrict__ y, const double *__restrict__ w_in, int n, int d,
    int npad, int mode, int maxiter, double tol, double etol, int emaxiter, double creg,
    double *__restrict__ theta_out, double *__restrict__ w_out, double *__restrict__ losses_out,
    int32_t *__restrict__ info, int32_t *__restrict__ status, unsigned long long *__restrict__ dbg) {
    extern __shared__ double sm[];
    LgShared sh;
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;                   // (64-bit offsets: B n d passes 2^31)
        X += b * (size_t)n * (size_t)d;
        y += b * (size_t)n;
        theta_out += b * (size_t)(d + 1);
        w_out += b * (size_t)n;
        if (losses_out != nullptr) losses_out += b * (size_t)n;
        info += b * 4;
    }
#if RLVI_STAMPS
    sh.dbg = dbg;
    sh.nst = (BATCH && blockIdx.x != 0) ? (1 << 30) : 0;      // only workgroup 0 leaves stamps
#else
    (void)dbg;
#endif
    sh.zsh = sm;
    sh.hsh = sh.zsh + npad;
    sh.csh = sh.hsh + npad;
    sh.gv = sh.csh + npad;
    sh.dl = sh.gv + SL_DP;
    sl_solve_carve(sh, sm + lg_solve_off(npad));
    const int tid = threadIdx.x;
    const int D = d + 1;
    int parity = 0;

    // the thread's samples: s = 2 y - 1, the weight (ones: rlvi.py:93), and whether they are what they must be
    double sgn[E], w[E], cw[E];
    double wmax = 0.0, nbad = 0.0, none = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        const bool v = q < n;
        const double yv = y[v ? q : 0];
        const double wv = (mode != 0) ? w_in[v ? q : 0] : 1.0;
        sgn[j] = yv == 1.0 ? 1.0 : -1.0;
        w[j] = v ? wv : 0.0;
        if (v && (!(yv == 0.0 || yv == 1.0) || !(wv >= 0.0 && wv < __builtin_inf()))) nbad += 1.0;
        wmax = w[j] > wmax ? w[j] : wmax;
    }
    for (int q = tid; q < 2 * SL_DP; q += SL_THREADS) sh.th[q] = 0.0;
    for (int q = tid; q < SL_DP * SL_GPITCH; q += SL_THREADS) sh.G[q] = 0.0;
    sl_block_sum2(nbad, none, sh.slots, parity);
    wmax = sl_block_max(wmax, sh.slots, parity);
    bool ok = nbad == 0.0 && wmax > 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) cw[j] = creg * (w[j] / wmax);                    // utils.py:66: weights / max

    int outer = 0, inner_last = 0, newton = 0;
    bool capped = false;
    while (ok) {
        LG_STAMP(0);   // outer iteration starts
        const int rc = lg_fit<E, DS, NB>(sh, X, n, d, sgn, cw, parity, newton);      // rlvi.py:94 the first time, then :101
        if (rc == 1) { ok = false; break; }
        capped = capped || rc == 2;
        if (mode != 0) break;
        if (outer > 0 && !sl_theta_moved(sh.th, D, tol)) break;      // rlvi.py:104-106
        if (outer >= maxiter) break;
        ++outer;
        // ---- update_weights(losses) (rlvi.py:98 -> :8-20); losses = -log p(class 0 | x) = log(1 + exp(z)) for every
        // sample, whatever y is (utils.py:62-64)
        double e[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            const bool v = q < n;
            const double z = sh.zsh[v ? q : 0];
            e[j] = v ? exp(-lg_softplus_neg(-z, exp(-fabs(z)))) : 0.0;
            w[j] = v ? 0.95 : 0.0;                                  // rlvi.py:10
        }
        LG_STAMP(8);   // exp done
        inner_last = sl_estep_fixed_point<E>(e, w, n, etol, emaxiter, sh.slots, parity);
        LG_STAMP(9);   // E-step done
        wmax = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) wmax = w[j] > wmax ? w[j] : wmax;
        wmax = sl_block_max(wmax, sh.slots, parity);
        if (!(wmax > 0.0)) { ok = false; break; }
#pragma unroll
        for (int j = 0; j < E; ++j) cw[j] = creg * (w[j] / wmax);
        if (tid < SL_DP) sh.th[SL_DP + tid] = sh.th[tid];          // prev_theta (rlvi.py:100)
        __syncthreads();
    }
    if (ok) {
        // theta = [intercept, coef ...] (utils.py:69)
        if (tid < D) theta_out[tid == d ? 0 : tid + 1] = sh.th[tid];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) {
                if (mode == 0) w_out[q] = w[j];
                const double z = sh.zsh[q];
                if (losses_out != nullptr) losses_out[q] = lg_softplus_neg(-z, exp(-fabs(z)));
            }
        }
    }
    if (tid == 0) {
        info[0] = outer;
        info[1] = inner_last;
        info[2] = newton;
        info[3] = !ok ? 1 : (capped ? 2 : 0);
        if (ok && capped) atomicOr(status, RLVI_ST_NOCONV);
    }
}

static int lg_check(int64_t n, int64_t d) {
    if (n <= 0 || d <= 0) return RLVI_E_SHAPE;
    return (n <= SL_MAXN && d <= LG_MAXD) ? 0 : RLVI_E_LIMIT;
}

// all three entries: mode 0 with one workgroup or (BATCH) one per problem of the batch, mode 1 (w_in the weights, no
// w_out) with one.  `required` is the entry's own list; the rest of the contract is the same.
template <bool BATCH>
static int lg_entry(std::initializer_list<const void *> required, const double *X, const double *y,
                    const double *w_in, int64_t batch, int64_t n, int64_t d, int mode, int maxiter, double tol,
                    double etol, int emaxiter, double creg, double *theta, double *w_out, double *losses, int32_t *info,
                    void *ws, void *stream) {
    if (const int e = sl_check_args(required, batch, n, d, maxiter >= 0 && emaxiter >= 0 && creg > 0.0,
                                    n <= SL_MAXN && d <= LG_MAXD, {X, y, w_in, theta, w_out, losses}, {info}, ws))
        return e;
    const int npad = sl_pad64(n);
    return sl_logreg_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(logreg_rlvi_kernel<F::E, F::DS, F::NB, BATCH>, batch, lg_lds_doubles(npad) * sizeof(double),
                         static_cast<hipStream_t>(stream), X, y, w_in, (int)n, (int)d, npad, mode, maxiter, tol, etol,
                         emaxiter, creg, theta, w_out, losses, info, sl_status(ws), stamp_base(ws));
    });
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_logistic_regression_check(int64_t n, int64_t d) { return lg_check(n, d); }

extern "C" int rlvi_logistic_regression_f64(const double *X, const double *y, int64_t n, int64_t d, int maxiter,
                                            double tol, double estep_tol, int estep_maxiter, double C, double *theta,
                                            double *weights, double *losses, int32_t *info, void *ws, void *stream) {
    return lg_entry<false>({X, y, theta, weights, info, ws}, X, y, nullptr, 1, n, d, 0, maxiter, tol, estep_tol,
                           estep_maxiter, C, theta, weights, losses, info, ws, stream);
}

extern "C" int rlvi_logistic_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                                  int maxiter, double tol, double estep_tol, int estep_maxiter,
                                                  double C, double *theta, double *weights, double *losses,
                                                  int32_t *info, void *ws, void *stream) {
    return lg_entry<true>({X, y, theta, weights, info, ws}, X, y, nullptr, batch, n, d, 0, maxiter, tol, estep_tol,
                          estep_maxiter, C, theta, weights, losses, info, ws, stream);
}

extern "C" int rlvi_logistic_fit_f64(const double *X, const double *y, const double *w, int64_t n, int64_t d, double C,
                                     double *theta, double *losses, int32_t *info, void *ws, void *stream) {
    return lg_entry<false>({X, y, w, theta, losses, info, ws}, X, y, w, 1, n, d, 1, 0, 0.0, 0.0, 0, C, theta, nullptr,
                           losses, info, ws, stream);
}
