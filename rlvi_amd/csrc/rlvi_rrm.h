// Robust Risk Minimization's weight rule (standard-learning/rrm.py:12-33) as an exact root, ONE copy: moments.hip (mean,
// PCA, covariance, the rule on its own), robust_linreg.hip (linear regression) and robust_logreg.hip (logistic
// regression) call it, each with the stride of its own slot area.
#pragma once
#include "rlvi_sl.h"

namespace rlvi {

constexpr int MO_ROOT_CAP = 200;                   // evaluations of one root-find
constexpr double MO_XI_MIN = -700.0, MO_XI_MAX = 700.0;   // xi = log alpha of the RRM rule: alpha stays a normal number
constexpr double MO_TMAX = 800.0;                  // exp(-800) is 0: a larger l / alpha is cut here (phi t = 0, never 0 inf)

// the eps the RRM regressions' entries take (what rlvi_amd.standard._rrm_eps accepts): RLVI_E_SHAPE otherwise
inline bool rl_eps_ok(double eps, int64_t n) { return eps > 0.0 && eps < 1.0 && (1.0 - eps) * (double)n > 1.0; }

// rrm.update_weights (rrm.py:12-33) on this thread's samples. The reference minimises g(alpha) = alpha (log sum_i
// exp(-l_i / alpha) - log((1 - eps) n)) over alpha = exp(xi) by scipy's Brent search and returns w_i = exp(-l_i / alpha)
// / sum_j exp(-l_j / alpha).  g is convex and stationary where the entropy of w equals log((1 - eps) n):
//     H(xi) = log S + (sum phi_i t_i) / S = log((1 - eps) n),  t_i = (l_i - min l) / alpha, phi_i = exp(-t_i), S = sum phi_i
// (the shift by min l moves g by a constant, leaves w as it is and makes every form overflow-safe: a covariance's
// losses are negative whenever log det is; S >= 1, so the reference's floor of 1e-16 under every phi is not needed and
// is DROPPED -- DESIGN 3.4f).  H increases in xi from log m, m the samples tied at the minimum, to log n, and dH/dxi =
// Var_w(t): the CONTRACT is that root, not Brent's iterate.  From xi = log mean(l - min l) a bracket is grown
// geometrically (steps 1, 2, 4, ...), then Newton steps, bisection where a step leaves the bracket or shrinks it too
// slowly; stops when the bracket is one ulp wide, the step is below one ulp or |H - target| <= 16 eps (1 + target): log
// S and the mean of t, each at most 1 + target here, carry the rounding of a sum of E + 8 terms per lane and wave.
// Each evaluation is the samples' arithmetic (one exp each) + ONE block sum of {S, sum phi t, sum phi t^2}.
// m >= (1 - eps) n, or no sign change down to MO_XI_MIN: there is no root, the minimiser runs off to alpha -> 0 and
// the rule returns that limit, 1 / m on the minima and 0 elsewhere (had_root false; all-equal losses are m = n).
// Returns 0, 1 (a loss that is not finite: w untouched) or 2 (MO_ROOT_CAP evaluations).  All threads call.
// `slots`: the caller's slot area of stride STRIDE >= 3 (sl_slot_doubles(STRIDE)) and its parity.
template <int E, int STRIDE>
__device__ __forceinline__ int mo_estep_rrm(const double (&l)[E], double (&w)[E], int n, double eps,
                                            double *slots, int &parity, int &evals, bool &had_root) {
    const int tid = threadIdx.x;
    evals = 0;
    had_root = false;
    double lmin = __builtin_inf(), none = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        lmin = (v && l[j] < lmin) ? l[j] : lmin;
    }
    sl_block_minmax<STRIDE>(lmin, none, slots, parity);
    double l0[E], phi[E], c[3] = {0.0, 0.0, 0.0};                  // c: ties at the minimum, sum l0, losses not finite
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        const double dl = l[j] - lmin;
        l0[j] = v ? dl : 0.0;
        phi[j] = (v && dl == 0.0) ? 1.0 : 0.0;
        c[0] += phi[j];
        c[1] += l0[j];
        c[2] += (v && !(fabs(dl) < __builtin_inf())) ? 1.0 : 0.0;
    }
    sl_block_sum<3, STRIDE>(c, slots, parity);
    if (c[2] != 0.0) return 1;
    const double keep = (1.0 - eps) * (double)n, target = log(keep), m = c[0];
    bool root = m < keep;
    double S = m;
    int rc = 0;
    if (root) {
        double s = log(c[1] / (double)n);
        s = (s > MO_XI_MIN) ? s : MO_XI_MIN;
        s = (s < MO_XI_MAX) ? s : MO_XI_MAX;
        const double gtol = 16.0 * SL_EPS * (1.0 + target);
        double lo = MO_XI_MIN, hi = MO_XI_MAX, grow = 1.0, dxold = 0.0, dx = 0.0;
        bool has_lo = false, has_hi = false;
        for (;;) {
            const double inva = exp(-s);
            double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool v = tid + j * SL_THREADS < n;
                double t = l0[j] * inva;
                t = (t < MO_TMAX) ? t : MO_TMAX;
                const double p = v ? exp(-t) : 0.0;
                phi[j] = p;
                a[0] += p;
                a[1] = __builtin_fma(p, t, a[1]);
                a[2] = __builtin_fma(p * t, t, a[2]);
            }
            sl_block_sum<3, STRIDE>(a, slots, parity);
            ++evals;
            S = a[0];
            const double mt = a[1] / S;
            const double f = log(S) + mt - target, fp = a[2] / S - mt * mt;
            if (fabs(f) <= gtol) break;
            const bool bracketed = has_lo && has_hi;
            if (f < 0.0) { lo = s; has_lo = true; } else { hi = s; has_hi = true; }
            if (evals >= MO_ROOT_CAP) { rc = 2; break; }
            double sn;
            if (!(has_lo && has_hi)) {
                if (f < 0.0) {
                    if (s >= MO_XI_MAX) break;                      // (losses of 1e300: the widest alpha is the answer)
                    sn = s + grow;
                    sn = (sn < MO_XI_MAX) ? sn : MO_XI_MAX;
                } else {
                    if (s <= MO_XI_MIN) { root = false; break; }    // the bracket's lower end is above the target
                    sn = s - grow;
                    sn = (sn > MO_XI_MIN) ? sn : MO_XI_MIN;
                }
                grow *= 2.0;
            } else {
                if (!bracketed) { dxold = hi - lo; dx = dxold; }
                sn = s - f / fp;
                if (fp > 0.0 && sn == s) break;                     // the Newton step is below one ulp of xi
                if (!(fp > 0.0) || !(sn > lo && sn < hi) || fabs(2.0 * f) > fabs(dxold * fp)) {
                    dxold = dx;
                    dx = 0.5 * (hi - lo);
                    sn = lo + dx;
                } else {
                    dxold = dx;
                    dx = fabs(sn - s);
                }
                if (sn == lo || sn == hi) break;                    // the bracket is one ulp wide
            }
            s = sn;
        }
    }
    if (!root) {
        S = m;
#pragma unroll
        for (int j = 0; j < E; ++j) phi[j] = (tid + j * SL_THREADS < n && l0[j] == 0.0) ? 1.0 : 0.0;
    }
    had_root = root;
#pragma unroll
    for (int j = 0; j < E; ++j) w[j] = phi[j] / S;                  // rrm.py:27-32 (every exit left phi and S at one xi)
    return rc;
}

}  // namespace rlvi
