// RRM's logistic regression, the last estimator of the reference's rrm.py, as ONE launch:
//
//   rlvi_rrm_logistic_regression_f64         standard-learning/rrm.py:76-91   logistic_regression(X, y, eps, maxiter, tol)
//   rlvi_rrm_logistic_regression_batch_f64   the sweep of standard-learning/main.py:361-470 around it
//
// The reference alternates scipy's Brent search (update_weights, rrm.py:12-33) with a liblinear fit (utils.py:61-73)
// on 100 .. 200 x 2 designs, up to 101 fits per call.  Both halves are on the device already, one copy of each:
// the weighted fit is lg_fit (rlvi_logreg.h: damped Newton on the matrix cores, to the minimiser liblinear
// approximates), the weight rule is mo_estep_rrm (rlvi_rrm.h: the exact entropy root).  This kernel keeps the two in
// one persistent workgroup of four waves with the LDS block of logreg_rlvi_kernel (logreg.hip), its dispatch table
// (sl_logreg_form, rlvi_sl_launch.h) and the rule's slot area, with a parity of its own, behind it.  Every decision is
// taken by every thread from the same LDS totals; sums are fp64 in a fixed order: same inputs, same bits.  Everything
// read from LDS is written by this workgroup first.
#include "rlvi_logreg.h"
#include "rlvi_rrm.h"
#include "rlvi_sl_launch.h"

namespace rlvi {

constexpr int RG_STRIDE = 3;                                      // values of the RRM rule's block sums
__host__ __device__ constexpr size_t rg_lds_doubles(int npad) { return lg_lds_doubles(npad) + sl_slot_doubles(RG_STRIDE); }

// rrm.logistic_regression (rrm.py:76-91 on utils.py:61-73) -> theta [d + 1] = (intercept, coef), weights [n] (the last
// rule's output; 1 / n with maxiter = 0).  info = { outer iterations, evaluations of the last root-find, Newton steps
// in all, flag }; flag 1: a label that is not 0 / 1 or a value that is not finite -- nothing written; 2: a fit ended at
// LG_NEWTON_CAP or without an acceptable Armijo step; 3: a root-find hit MO_ROOT_CAP (2 and 3: RLVI_ST_NOCONV in the
// workspace, the results written; 2 is reported before 3).  Reaching maxiter is silent, as in the reference.
// BATCH: workgroup b works on problem b of a contiguous batch (X [B, n, d], y [B, n], theta [B, d + 1], weights [B, n],
// info [B, 4]) behind wave-uniform pointer offsets; `status` is the ONE word of the workspace for all workgroups.
template <int E, int DS, int NB, bool BATCH>
__global__ __launch_bounds__(SL_THREADS) void logreg_rrm_kernel(
    const double *__restrict__ X, const double *__restrict__ y, int n, int d, int npad, int maxiter, double tol,
    double eps, double creg, double *__restrict__ theta_out, double *__restrict__ w_out, int32_t *__restrict__ info,
    int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;                   // (64-bit offsets: B n d passes 2^31)
        X += b * (size_t)n * (size_t)d;
        y += b * (size_t)n;
        theta_out += b * (size_t)(d + 1);
        w_out += b * (size_t)n;
        info += b * 4;
    }
    LgShared sh;
#if RLVI_STAMPS
    sh.dbg = nullptr;
    sh.nst = 1 << 30;                                  // (this kernel leaves no stamps)
#endif
    sh.zsh = sm;
    sh.hsh = sh.zsh + npad;
    sh.csh = sh.hsh + npad;
    sh.gv = sh.csh + npad;
    sh.dl = sh.gv + SL_DP;
    sl_solve_carve(sh, sm + lg_solve_off(npad));
    double *const slots3 = sm + lg_lds_doubles(npad);
    const int tid = threadIdx.x;
    const int D = d + 1;
    int parity = 0, parity3 = 0;

    // the thread's samples: s = 2 y - 1, and whether the labels are what they must be.  Weights 1 / n (rrm.py:77):
    // w / max w = 1, so C what = C (utils.py:66)
    double sgn[E], w[E], cw[E];
    double nbad = 0.0, none = 0.0;
    const double w0 = 1.0 / (double)n;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        const bool v = q < n;
        const double yv = y[v ? q : 0];
        sgn[j] = yv == 1.0 ? 1.0 : -1.0;
        w[j] = v ? w0 : 0.0;
        cw[j] = v ? creg : 0.0;
        if (v && !(yv == 0.0 || yv == 1.0)) nbad += 1.0;
    }
    for (int q = tid; q < 2 * SL_DP; q += SL_THREADS) sh.th[q] = 0.0;
    for (int q = tid; q < SL_DP * SL_GPITCH; q += SL_THREADS) {
        sh.G[q] = 0.0;
        sh.LT[q] = 0.0;                                // (a lane beyond the padded system reads rows no factorisation writes)
    }
    sl_block_sum2(nbad, none, sh.slots, parity);

    int outer = 0, evals_last = 0, newton = 0, flag = nbad == 0.0 ? 0 : 1;
    bool capped_fit = false, capped_root = false;
    while (flag == 0) {
        // (ONE call site for the fit, as in logreg_rlvi_kernel: rrm.py:78 the first time, then :84)
        int rc = lg_fit<E, DS, NB>(sh, X, n, d, sgn, cw, parity, newton);
        if (rc == 1) { flag = 1; break; }
        capped_fit = capped_fit || rc == 2;
        if (outer > 0 && !sl_theta_moved(sh.th, D, tol)) break;      // rrm.py:87-89 (||prev|| = 0: NaN, no stop)
        if (outer >= maxiter) break;                                 // rrm.py:80: silent
        ++outer;
        // losses = -log p(class 0 | x) = log(1 + exp(z)) for every sample, whatever y is (utils.py:62-64)
        double l[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            const bool v = q < n;
            const double z = sh.zsh[v ? q : 0];
            l[j] = v ? lg_softplus_neg(-z, exp(-fabs(z))) : 0.0;
        }
        bool had_root;
        rc = mo_estep_rrm<E, RG_STRIDE>(l, w, n, eps, slots3, parity3, evals_last, had_root);          // rrm.py:81
        if (rc == 1) { flag = 1; break; }
        capped_root = capped_root || rc == 2;
        double wmax = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) wmax = w[j] > wmax ? w[j] : wmax;
        wmax = sl_block_max(wmax, sh.slots, parity);
        if (!(wmax > 0.0)) { flag = 1; break; }
#pragma unroll
        for (int j = 0; j < E; ++j) cw[j] = creg * (w[j] / wmax);                        // utils.py:66: weights / max
        if (tid < SL_DP) sh.th[SL_DP + tid] = sh.th[tid];            // prev_theta (rrm.py:83)
        __syncthreads();
    }
    if (flag == 0) {
        // theta = [intercept, coef ...] (utils.py:69)
        if (tid < D) theta_out[tid == d ? 0 : tid + 1] = sh.th[tid];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) w_out[q] = w[j];
        }
    }
    if (tid == 0) {
        const bool capped = capped_fit || capped_root;
        info[0] = outer;
        info[1] = evals_last;
        info[2] = newton;
        info[3] = flag != 0 ? flag : (capped_fit ? 2 : (capped_root ? 3 : 0));
        if (flag == 0 && capped) atomicOr(status, RLVI_ST_NOCONV);
    }
}

// both entries: one workgroup, or (BATCH) one per problem of the batch.  The contract of
// rlvi_logistic_regression_f64 and the eps rule of the RRM regressions; sl_logreg_form is logreg.hip's table.
template <bool BATCH>
static int rg_entry(const double *X, const double *y, int64_t batch, int64_t n, int64_t d, double eps,
                    int maxiter, double tol, double creg, double *theta, double *weights, int32_t *info, void *ws,
                    void *stream) {
    if (const int e = sl_check_args({X, y, theta, weights, info, ws}, batch, n, d,
                                    maxiter >= 0 && creg > 0.0 && rl_eps_ok(eps, n), n <= SL_MAXN && d <= LG_MAXD,
                                    {X, y, theta, weights}, {info}, ws))
        return e;
    const int npad = sl_pad64(n);
    return sl_logreg_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(logreg_rrm_kernel<F::E, F::DS, F::NB, BATCH>, batch, rg_lds_doubles(npad) * sizeof(double),
                         static_cast<hipStream_t>(stream), X, y, (int)n, (int)d, npad, maxiter, tol, eps, creg, theta,
                         weights, info, sl_status(ws));
    });
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_rrm_logistic_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double eps,
                                                int maxiter, double tol, double C, double *theta, double *weights,
                                                int32_t *info, void *ws, void *stream) {
    return rg_entry<false>(X, y, 1, n, d, eps, maxiter, tol, C, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_logistic_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n,
                                                      int64_t d, double eps, int maxiter, double tol, double C,
                                                      double *theta, double *weights, int32_t *info, void *ws,
                                                      void *stream) {
    return rg_entry<true>(X, y, batch, n, d, eps, maxiter, tol, C, theta, weights, info, ws, stream);
}
