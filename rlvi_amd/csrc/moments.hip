// RLVI's mean, PCA and covariance estimators as ONE launch each (the last three of standard-learning/rlvi.py), and the
// constrained E-step on its own:
//
//   rlvi_robust_mean_f64                   standard-learning/rlvi.py:46-65     mean(sample, maxiter, tol)
//   rlvi_robust_pca_f64                    rlvi.py:111-125, utils.py:76-89     pca(sample, maxiter, tol, theta_init)
//   rlvi_robust_covariance_f64             rlvi.py:128-144, utils.py:92-108    covariance(sample, eps, maxiter, tol)
//   rlvi_update_weights_constrained_f64    rlvi.py:23-43                       update_weights_constrained(losses, n_eff)
//
// and the same three under Robust Risk Minimization (standard-learning/rrm.py), the competitor the reference's
// experiments plot beside them: the outer loops above with another weight rule (mo_estep_rrm) and 1 / n as first weights:
//
//   rlvi_rrm_mean_f64                      standard-learning/rrm.py:36-52      mean(sample, eps, maxiter, tol)
//   rlvi_rrm_pca_f64                       rrm.py:94-107, utils.py:76-89       pca(sample, eps, maxiter, tol, theta_init)
//   rlvi_rrm_covariance_f64                rrm.py:110-124, utils.py:92-108     covariance(sample, eps, maxiter, tol)
//   rlvi_rrm_update_weights_f64            rrm.py:12-33                        update_weights(losses, eps)
//
// The reference runs them on 100 x 2, 40 x 2 and 50 x 2 samples for 2 .. 8 outer iterations: latency that a launch, a
// copy or a third-party call per statement can never amortise (DESIGN, "Mean, PCA and covariance in one launch").
//
// One persistent workgroup of four waves, as linreg_rlvi_kernel (standard.hip) and logreg_rlvi_kernel (logreg.hip):
//   * the sample [n, d] is staged into LDS once and every pass reads it from there; thread tid owns the samples
//     tid + 256 j and keeps their weights and losses in registers;
//   * weighted moments are TWO passes -- sum a and sum a x, then sum a (x - m)(x - m)^T about the mean just found (never
//     S2 - m m^T: a cloud at 1e6 with unit spread would lose twelve digits) --, each ONE block sum of K values behind
//     one barrier (sl_block_sum<K>);
//   * the d x d algebra (d <= 8, padded to 2 / 4 / 8) runs on EVERY thread, redundantly, in registers, from the same
//     LDS totals: an L D L^T factorisation with the pivot test of sl_ldlt_solve (covariance), cyclic Jacobi sweeps
//     (PCA) -- no broadcast, no further barrier;
//   * the constrained E-step finds the root s of sum_i 1 / (1 + c exp(l_i - s)) = n_eff, c = (n - n_eff) / n_eff, by
//     safeguarded Newton on the bracket [min l, max l]: the exact root of what the reference hands to scipy's Brent
//     search as a square.  The CONTRACT is the root, not Brent's iterate;
//   * every decision (E-step stop, root-find stop, Jacobi stop, outer stop) is taken by every thread from the same
//     LDS totals: no host in the loop, one launch, the host waits once.
// Sums are fp64 in a fixed order: same inputs, same bits.
// PCA: an exactly repeated largest eigenvalue leaves the direction unpinned (any vector of its eigenspace is an
// answer; the one returned is what the sweeps happen to leave).
#include "rlvi_rrm.h"
#include "rlvi_sl_launch.h"

namespace rlvi {

constexpr int MO_MAXD = 8;
constexpr int MO_MAXND = 16384;                    // n d doubles of the sample resident in LDS: 128 KB
constexpr int MO_KMAX = 36;                        // values of one block sum: the lower triangle of 8 x 8
constexpr int MO_JACOBI_CAP = 30;                  // sweeps of one eigen-solve
constexpr double MO_EPS = SL_EPS;

struct MoShared {
    const double *xs;   // [n * d] the sample
    double *slots;      // [2][SL_NW][MO_KMAX]  every block reduction of these kernels, the E-step's included
};

__host__ __device__ constexpr int mo_tri(int i, int j) { return i * (i + 1) / 2 + j; }     // j <= i

// row q of the sample, 0 beyond its d columns and for a sample past n
template <int DS>
__device__ __forceinline__ void mo_row(const double *xs, int q, int d, bool valid, double (&x)[DS]) {
#pragma unroll
    for (int c = 0; c < DS; ++c) {
        const bool in = valid && c < d;
        const double v = xs[in ? q * d + c : 0];
        x[c] = in ? v : 0.0;
    }
}

// The eigenvector of the largest eigenvalue of the symmetric positive semi-definite A (lower triangle a2, 0 beyond
// its d rows) by cyclic Jacobi sweeps until the off-diagonal mass is at the rounding floor, normalised, its component
// of largest magnitude (the first on a tie) positive: sklearn's svd_flip(u_based_decision=False).  Every thread runs it
// on the same numbers.  Returns 0, 1 (A not finite) or 2 (MO_JACOBI_CAP sweeps without reaching the floor).
template <int DS>
__device__ __forceinline__ int mo_jacobi_top(const double (&a2)[DS * (DS + 1) / 2], int d, double (&th)[DS],
                                             int &sweeps) {
    double a[DS][DS], v[DS][DS];
    double fro2 = 0.0;
#pragma unroll
    for (int i = 0; i < DS; ++i) {
#pragma unroll
        for (int j = 0; j < DS; ++j) {
            a[i][j] = j <= i ? a2[mo_tri(i, j)] : a2[mo_tri(j, i)];
            v[i][j] = i == j ? 1.0 : 0.0;
            fro2 = __builtin_fma(a[i][j], a[i][j], fro2);
        }
    }
    if (!(fro2 < __builtin_inf())) return 1;
    // the floor: a rotation leaves each entry within eps |A| of its exact value
    const double thr = (double)(DS * DS) * MO_EPS;
    int rc = 0;
    for (int sweep = 0;; ++sweep) {
        double off2 = 0.0;
#pragma unroll
        for (int p = 0; p < DS; ++p) {
#pragma unroll
            for (int q = p + 1; q < DS; ++q) off2 = __builtin_fma(a[p][q], a[p][q], off2);
        }
        if (off2 <= thr * thr * fro2) break;
        if (sweep >= MO_JACOBI_CAP) { rc = 2; break; }
        ++sweeps;
#pragma unroll
        for (int p = 0; p < DS; ++p) {
#pragma unroll
            for (int q = p + 1; q < DS; ++q) {
                const double apq = a[p][q];
                if (apq != 0.0) {                                   // (the same on every thread)
                    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                    const double t = __builtin_copysign(1.0, theta) / (fabs(theta) + sqrt(__builtin_fma(theta, theta, 1.0)));
                    const double c = 1.0 / sqrt(__builtin_fma(t, t, 1.0));
                    const double s = t * c, tau = s / (1.0 + c);
                    a[p][p] -= t * apq;
                    a[q][q] += t * apq;
                    a[p][q] = 0.0;
                    a[q][p] = 0.0;
#pragma unroll
                    for (int r = 0; r < DS; ++r) {
                        if (r != p && r != q) {
                            const double arp = a[r][p], arq = a[r][q];
                            a[r][p] = arp - s * (arq + tau * arp);
                            a[p][r] = a[r][p];
                            a[r][q] = arq + s * (arp - tau * arq);
                            a[q][r] = a[r][q];
                        }
                        const double vrp = v[r][p], vrq = v[r][q];
                        v[r][p] = vrp - s * (vrq + tau * vrp);
                        v[r][q] = vrq + s * (vrp - tau * vrq);
                    }
                }
            }
        }
    }
    // the largest eigenvalue among the d real ones (the first on a tie), its column of V
    int k = 0;
    double best = a[0][0];
#pragma unroll
    for (int c = 1; c < DS; ++c) {
        if (c < d && a[c][c] > best) { best = a[c][c]; k = c; }
    }
    double nrm2 = 0.0;
#pragma unroll
    for (int r = 0; r < DS; ++r) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < DS; ++c) t = c == k ? v[r][c] : t;
        th[r] = t;
        nrm2 = __builtin_fma(t, t, nrm2);
    }
    const double nrm = sqrt(nrm2);
    double big = -1.0, sign = 1.0;
#pragma unroll
    for (int r = 0; r < DS; ++r) {
        th[r] /= nrm;                                                // utils.py:85
        if (r < d && fabs(th[r]) > big) { big = fabs(th[r]); sign = th[r] < 0.0 ? -1.0 : 1.0; }
    }
#pragma unroll
    for (int r = 0; r < DS; ++r) th[r] *= sign;
    return rc;
}

template <int MODE, int DS> struct MoTheta { static constexpr int N = MODE == 2 ? DS * (DS + 1) / 2 : DS; };

// One M-step: theta from the weights w of this thread's samples, and their losses l.
//   MODE 0  rlvi.py:48-51 / :56-59     theta = sum w x / sum w, r = ||theta - x||^2, losses = 1/2 r / (sum w r / sum w)
//           RRM (rrm.py:38-39 / :45-46): losses = r, no variance
//   MODE 1  utils.py:76-89             theta = first principal component of the rows w x (skipped: `given`, theta is
//                                      the caller's), losses = ||x||^2 - (x.theta)^2
//           RRM: (x.theta)^2 is rounded before it is subtracted, never fused into the subtraction -- at d = 1 the loss
//           is then exactly 0, as it is in exact arithmetic, and not the product's rounding error: RRM's rule is
//           scale-free, and would turn that noise into weights
//   MODE 2  utils.py:92-108            theta = the weighted covariance (lower triangle), losses = 1/2 ((x - mu)^T
//                                      C^-1 (x - mu) + log det C + d log 2 pi)
// Returns, on every thread, 0, 1 (numbers that are not finite, no positive weight, a variance or a pivot not safely
// positive) or 2 (the Jacobi cap).  All threads call.
template <int MODE, int E, int DS, bool RRM = false>
__device__ __forceinline__ int mo_fit(const MoShared &sh, int n, int d, const double (&w)[E], double (&l)[E],
                                      double (&th)[MoTheta<MODE, DS>::N], bool given, int &parity, int &sweeps) {
    constexpr int NTRI = DS * (DS + 1) / 2;
    const int tid = threadIdx.x;
    int rc = 0;
    if (!(MODE == 1 && given)) {
        // ---- pass 1: sum w, sum w x
        double s1[1 + DS];
#pragma unroll
        for (int k = 0; k < 1 + DS; ++k) s1[k] = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            double x[DS];
            mo_row<DS>(sh.xs, q, d, q < n, x);
            s1[0] += w[j];
#pragma unroll
            for (int c = 0; c < DS; ++c) s1[1 + c] = __builtin_fma(w[j], x[c], s1[1 + c]);
        }
        sl_block_sum<1 + DS, MO_KMAX>(s1, sh.slots, parity);
        const double s0 = s1[0];
        if (!(s0 > 0.0 && s0 < __builtin_inf())) return 1;
        double m[DS];
        const double den = MODE == 1 ? (double)n : s0;              // utils.py:83: PCA centres by the plain column mean
#pragma unroll
        for (int c = 0; c < DS; ++c) m[c] = s1[1 + c] / den;
        if (MODE == 0) {
            double swr = 0.0, none = 0.0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                double x[DS];
                mo_row<DS>(sh.xs, q, d, q < n, x);
                double r = 0.0;
#pragma unroll
                for (int c = 0; c < DS; ++c) r = __builtin_fma(m[c] - x[c], m[c] - x[c], r);
                l[j] = q < n ? r : 0.0;
                swr = __builtin_fma(w[j], l[j], swr);
            }
            if (!RRM) {
                sl_block_sum2<MO_KMAX>(swr, none, sh.slots, parity);
                const double sigma2 = swr / s0;
                if (!(sigma2 > 0.0 && sigma2 < __builtin_inf())) return 1;
#pragma unroll
                for (int j = 0; j < E; ++j) l[j] = 0.5 * l[j] / sigma2;
            }
#pragma unroll
            for (int c = 0; c < DS; ++c) th[c] = m[c];
            return 0;
        }
        // ---- pass 2: the second moment about the mean just found
        double a2[NTRI];
#pragma unroll
        for (int k = 0; k < NTRI; ++k) a2[k] = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            const bool valid = q < n;
            double x[DS], y[DS];
            mo_row<DS>(sh.xs, q, d, valid, x);
#pragma unroll
            for (int c = 0; c < DS; ++c) {
                y[c] = MODE == 1 ? __builtin_fma(w[j], x[c], -m[c]) : x[c] - m[c];
                if (MODE == 1) y[c] = valid ? y[c] : 0.0;
            }
#pragma unroll
            for (int c1 = 0; c1 < DS; ++c1) {
                const double yc = MODE == 1 ? y[c1] : w[j] * y[c1];
#pragma unroll
                for (int c2 = 0; c2 <= c1; ++c2) a2[mo_tri(c1, c2)] = __builtin_fma(yc, y[c2], a2[mo_tri(c1, c2)]);
            }
        }
        sl_block_sum<NTRI, MO_KMAX>(a2, sh.slots, parity);
        if (MODE == 1) {
            double t[DS];
            rc = mo_jacobi_top<DS>(a2, d, t, sweeps);
            if (rc == 1) return 1;
#pragma unroll
            for (int c = 0; c < DS; ++c) th[c] = t[c];
        }
        if (MODE == 2) {
            // C = the moment / sum w, padded with the identity; L D L^T in place with the pivot test of sl_ldlt_solve
            double g[NTRI], dinv[DS];
            double dmax = 0.0;
#pragma unroll
            for (int i = 0; i < DS; ++i) {
#pragma unroll
                for (int k = 0; k <= i; ++k) {
                    const double cv = a2[mo_tri(i, k)] / s0;
                    g[mo_tri(i, k)] = (i < d) ? cv : (i == k ? 1.0 : 0.0);
                    th[mo_tri(i, k)] = cv;
                }
                if (i < d) dmax = g[mo_tri(i, i)] > dmax ? g[mo_tri(i, i)] : dmax;
            }
            const double piv_min = sl_pivot_floor(dmax, d);
            bool bad = !(dmax < __builtin_inf());
            double logdet = 0.0;
#pragma unroll
            for (int j = 0; j < DS; ++j) {
                const double piv = g[mo_tri(j, j)];
                bad = bad || (j < d && !(piv > piv_min));
                const double inv = 1.0 / piv;
                dinv[j] = inv;
                logdet += (j < d && !bad) ? log(piv) : 0.0;
#pragma unroll
                for (int i = j + 1; i < DS; ++i) {
                    const double lij = g[mo_tri(i, j)] * inv;
#pragma unroll
                    for (int k = j + 1; k <= i; ++k)
                        g[mo_tri(i, k)] = __builtin_fma(-lij, g[mo_tri(k, j)], g[mo_tri(i, k)]);
                }
#pragma unroll
                for (int i = j + 1; i < DS; ++i) g[mo_tri(i, j)] *= inv;
            }
            if (bad) return 1;
            const double cst = logdet + (double)d * 1.8378770664093453;       // log 2 pi
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                double x[DS], z[DS];
                mo_row<DS>(sh.xs, q, d, q < n, x);
                double r = 0.0;
#pragma unroll
                for (int i = 0; i < DS; ++i) {
                    double zi = i < d ? x[i] - m[i] : 0.0;
#pragma unroll
                    for (int k = 0; k < i; ++k) zi = __builtin_fma(-g[mo_tri(i, k)], z[k], zi);
                    z[i] = zi;
                    r = __builtin_fma(zi * zi, dinv[i], r);
                }
                l[j] = q < n ? 0.5 * (r + cst) : 0.0;
            }
            return 0;
        }
    }
    // MODE 1: losses on the uncentred rows (utils.py:77-79)
    if (MODE == 1) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            double x[DS];
            mo_row<DS>(sh.xs, q, d, q < n, x);
            double ss = 0.0, p = 0.0;
#pragma unroll
            for (int c = 0; c < DS; ++c) {
                ss = __builtin_fma(x[c], x[c], ss);
                p = __builtin_fma(x[c], th[c], p);
            }
            if (RRM) {
                double pp = p * p;
                sl_keep(pp);
                l[j] = q < n ? ss - pp : 0.0;
            } else {
                l[j] = q < n ? ss - p * p : 0.0;
            }
        }
    }
    return rc;
}

// update_weights_constrained (rlvi.py:23-43) on this thread's samples: the plain fixed point first; if its weights
// sum to less than n_eff, the shift s with sum_i 1 / (1 + c exp(l_i - s)) = n_eff, c = (n - n_eff) / n_eff (the
// overflow-safe form: a loss of 1e12 gives the weight 0, never 0 / 0).  The sum is monotone in s and [min l, max l]
// brackets the root (at s = l_i the i-th term is n_eff / n): Newton steps, bisection where a step leaves the bracket
// or shrinks it too slowly; stops when the bracket is one ulp wide or |sum - n_eff| <= 4 n eps.  Each evaluation is
// the samples' arithmetic + one block sum.  inner: the fixed point's iterations; active: the constraint was;
// returns 0 or 2 (MO_ROOT_CAP evaluations).
template <int E>
__device__ __forceinline__ int mo_estep_constrained(const double (&l)[E], double (&w)[E], int n, double n_eff,
                                                    double etol, int emaxiter, const MoShared &sh, int &parity,
                                                    int &inner, bool &active, int &evals) {
    const int tid = threadIdx.x;
    double e[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        e[j] = v ? exp(-l[j]) : 0.0;
        w[j] = v ? 0.95 : 0.0;                                      // rlvi.py:10
    }
    inner = sl_estep_fixed_point<E, MO_KMAX>(e, w, n, etol, emaxiter, sh.slots, parity);
    double sum = 0.0, none = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) sum += w[j];
    sl_block_sum2<MO_KMAX>(sum, none, sh.slots, parity);
    active = sum < n_eff;                                           // rlvi.py:40
    evals = 0;
    if (!active) return 0;
    double lo = __builtin_inf(), hi = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        lo = (v && l[j] < lo) ? l[j] : lo;
        hi = (v && l[j] > hi) ? l[j] : hi;
    }
    sl_block_minmax<MO_KMAX>(lo, hi, sh.slots, parity);
    const double c = ((double)n - n_eff) / n_eff;
    // where the fixed point stopped: its weights are 1 / (1 + ratio exp(l)), i.e. the shift log(c / ratio)
    double s;
    { const double eps = 1.0 - sum / (double)n; s = log(c * (1.0 - eps) / eps); }
    s = (s > lo) ? s : lo;
    s = (s < hi) ? s : hi;
    const double gtol = 4.0 * (double)n * MO_EPS;
    double dxold = hi - lo, dx = dxold;
    int rc = 0;
    for (;;) {
        double g = 0.0, gp = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const bool v = tid + j * SL_THREADS < n;
            const double t = v ? 1.0 / (1.0 + c * exp(l[j] - s)) : 0.0;
            g += t;
            gp = __builtin_fma(t, 1.0 - t, gp);
        }
        sl_block_sum2<MO_KMAX>(g, gp, sh.slots, parity);
        ++evals;
        const double f = g - n_eff;
        if (fabs(f) <= gtol) break;
        if (f < 0.0) lo = s; else hi = s;
        if (evals >= MO_ROOT_CAP) { rc = 2; break; }
        double sn = s - f / gp;
        if (gp > 0.0 && sn == s) break;                             // the Newton step is below one ulp of s
        if (!(gp > 0.0) || !(sn > lo && sn < hi) || fabs(2.0 * f) > fabs(dxold * gp)) {
            dxold = dx;
            dx = 0.5 * (hi - lo);
            sn = lo + dx;
        } else {
            dxold = dx;
            dx = fabs(sn - s);
        }
        if (sn == lo || sn == hi) break;                            // the bracket is one ulp wide
        s = sn;
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        w[j] = v ? 1.0 / (1.0 + c * exp(l[j] - s)) : 0.0;           // rlvi.py:42
    }
    return rc;
}

// the kernels' LDS in doubles: the sample (an even count), then the slots
__host__ __device__ constexpr size_t mo_slots_off(int64_t nd) { return (size_t)((nd + 1) & ~(int64_t)1); }
__device__ __forceinline__ void mo_carve(MoShared &sh, double *sm, int nd) {
    sh.xs = sm;
    sh.slots = sm + mo_slots_off(nd);
}
static size_t mo_lds_bytes(int64_t nd) { return (mo_slots_off(nd) + sl_slot_doubles(MO_KMAX)) * sizeof(double); }

// MODE 0 / 1 / 2: mean / pca / covariance.  theta_out: [d], [d], [d * d]; info: { outer iterations, inner iterations of
// the last E-step, inner iterations in all | Jacobi sweeps in all | E-steps with the constraint active, flag }.
// MODE 3 / 4 / 5: the same three fits under RRM (rrm.py:36-52, :94-124) -- new MODE values and not a further template
// parameter, so that the RLVI instantiations keep their symbols and their instructions: first weights 1 / n, the weight
// rule mo_estep_rrm with eps in the place of n_eff, the fits' RRM forms (mo_fit); info: { outer iterations, evaluations of the
// last root-find, evaluations in all | Jacobi sweeps in all | evaluations in all, flag }; flag 1 as well for eps outside
// (0, 1), (1 - eps) n <= 1 and a loss that is not finite.
// BATCH: workgroup b works on problem b of a contiguous batch (X [B, n, d], theta [B, d] or [B, d * d], weights [B, n],
// info [B, 4]; theta_init and n_eff are the whole batch's) behind wave-uniform pointer offsets -- a template flag, as
// in linreg_rlvi_kernel: the single form keeps its instructions.  `status` is the ONE word of the workspace for all
// workgroups (atomicOr); a problem's own flag is info[4 b + 3].  LDS holds the sample, staged by this workgroup, and the
// slots, written before every read: nothing a CU's previous workgroup left behind is read.
template <int MODE, int E, int DS, bool BATCH = false>
__global__ __launch_bounds__(SL_THREADS) void moments_rlvi_kernel(
    const double *__restrict__ X, const double *__restrict__ theta_init, int n, int d, int maxiter, double tol,
    double etol, int emaxiter, double n_eff, double *__restrict__ theta_out, double *__restrict__ w_out,
    int32_t *__restrict__ info, int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    constexpr int FIT = MODE % 3;                      // which of the three fits
    constexpr bool RRM = MODE >= 3;
    constexpr int NT = MoTheta<FIT, DS>::N;
    if constexpr (BATCH) {
        const size_t b = blockIdx.x;                   // (64-bit offsets: B n d passes 2^31)
        X += b * (size_t)n * (size_t)d;
        theta_out += b * (size_t)(FIT == 2 ? d * d : d);
        w_out += b * (size_t)n;
        info += b * 4;
    }
    MoShared sh;
    mo_carve(sh, sm, n * d);
    const int tid = threadIdx.x;
    int parity = 0;

    // the sample -> LDS, and whether it is what it must be
    double nbad = 0.0, none = 0.0;
    for (int q = tid; q < n * d; q += SL_THREADS) {
        const double v = X[q];
        sm[q] = v;
        if (!(fabs(v) < __builtin_inf())) nbad += 1.0;
    }
    const bool given = FIT == 1 && theta_init != nullptr;
    double th[NT], prev[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) { th[k] = 0.0; prev[k] = 0.0; }
    if (given) {
#pragma unroll
        for (int c = 0; c < DS; ++c) {
            if (c < d) {
                th[c] = theta_init[c];
                if (!(fabs(th[c]) < __builtin_inf())) nbad += 1.0;
            }
        }
    }
    if (MODE == 2 && !(n_eff > 0.0 && n_eff < (double)n)) nbad += 1.0;
    if (RRM && !(n_eff > 0.0 && n_eff < 1.0 && (1.0 - n_eff) * (double)n > 1.0)) nbad += 1.0;    // (n_eff: eps)
    sl_block_sum2<MO_KMAX>(nbad, none, sh.slots, parity);                    // (its barrier publishes the sample)
    bool ok = nbad == 0.0;

    double w[E], l[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        // rlvi.py:47 / :112 / :132; rrm.py:37 / :95 / :111
        w[j] = (tid + j * SL_THREADS < n) ? (RRM ? 1.0 / (double)n : 1.0) : 0.0;
        l[j] = 0.0;
    }
    int outer = 0, inner_last = 0, count = 0;
    bool capped = false;
    if (ok) {
        const int rc = mo_fit<FIT, E, DS, RRM>(sh, n, d, w, l, th, given, parity, count);
        ok = rc != 1;
        capped = rc == 2;
    }
    while (ok && outer < maxiter) {
        ++outer;
        if (RRM) {
            bool had_root;
            const int rc = mo_estep_rrm<E, MO_KMAX>(l, w, n, n_eff, sh.slots, parity, inner_last, had_root);
            if (rc == 1) { ok = false; break; }
            capped = capped || rc == 2;
            if (FIT != 1) count += inner_last;
        } else if (MODE == 2) {
            bool active;
            int evals;
            const int rc = mo_estep_constrained<E>(l, w, n, n_eff, etol, emaxiter, sh, parity, inner_last, active,
                                                   evals);
            capped = capped || rc == 2;
            count += active ? 1 : 0;
        } else {
            double e[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const bool v = tid + j * SL_THREADS < n;
                e[j] = v ? exp(-l[j]) : 0.0;
                w[j] = v ? 0.95 : 0.0;                              // rlvi.py:10
            }
            inner_last = sl_estep_fixed_point<E, MO_KMAX>(e, w, n, etol, emaxiter, sh.slots, parity);
            if (MODE == 0) count += inner_last;
        }
#pragma unroll
        for (int k = 0; k < NT; ++k) prev[k] = th[k];
        const int rc = mo_fit<FIT, E, DS, RRM>(sh, n, d, w, l, th, false, parity, count);
        if (rc == 1) { ok = false; break; }
        capped = capped || rc == 2;
        // ||theta - prev|| / ||prev|| <= tol (the Frobenius norms of the full matrix for the covariance)
        double dn = 0.0, pn = 0.0;
        if (FIT == 2) {
#pragma unroll
            for (int i = 0; i < DS; ++i) {
#pragma unroll
                for (int k = 0; k <= i; ++k) {
                    const double df = th[mo_tri(i, k)] - prev[mo_tri(i, k)], pv = prev[mo_tri(i, k)];
                    const double twice = i == k ? 1.0 : 2.0;
                    dn = __builtin_fma(twice * df, df, dn);
                    pn = __builtin_fma(twice * pv, pv, pn);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                dn = __builtin_fma(th[k] - prev[k], th[k] - prev[k], dn);
                pn = __builtin_fma(prev[k], prev[k], pn);
            }
        }
        if (sqrt(dn) / sqrt(pn) <= tol) break;
    }
    if (ok) {
        if (tid == 0) {
            if (FIT == 2) {
#pragma unroll
                for (int i = 0; i < DS; ++i) {
#pragma unroll
                    for (int k = 0; k <= i; ++k) {
                        if (i < d) {
                            theta_out[i * d + k] = th[mo_tri(i, k)];
                            theta_out[k * d + i] = th[mo_tri(i, k)];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < DS; ++c) {
                    if (c < d) theta_out[c] = th[c];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) w_out[q] = w[j];
        }
    }
    if (tid == 0) {
        info[0] = outer;
        info[1] = inner_last;
        info[2] = count;
        info[3] = !ok ? 1 : (capped ? 2 : 0);
        if (ok && capped) atomicOr(status, RLVI_ST_NOCONV);
    }
}

// update_weights_constrained on its own: info = { root-find evaluations, the fixed point's iterations, 1 if the
// constraint was active, flag }
template <int E>
__global__ __launch_bounds__(SL_THREADS) void moments_uwc_kernel(const double *__restrict__ losses, int n, double n_eff,
                                                                 double etol, int emaxiter, double *__restrict__ out,
                                                                 int32_t *__restrict__ info,
                                                                 int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    MoShared sh;
    mo_carve(sh, sm, 0);
    const int tid = threadIdx.x;
    int parity = 0;
    double l[E], w[E];
    double nbad = 0.0, none = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        l[j] = losses[q < n ? q : 0];
        w[j] = 0.0;
        if (q < n && !(fabs(l[j]) < __builtin_inf())) nbad += 1.0;
    }
    if (!(n_eff > 0.0 && n_eff < (double)n)) nbad += 1.0;
    sl_block_sum2<MO_KMAX>(nbad, none, sh.slots, parity);
    const bool ok = nbad == 0.0;
    int inner = 0, evals = 0, rc = 0;
    bool active = false;
    if (ok) {
        rc = mo_estep_constrained<E>(l, w, n, n_eff, etol, emaxiter, sh, parity, inner, active, evals);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) out[q] = w[j];
        }
    }
    if (tid == 0) {
        info[0] = evals;
        info[1] = inner;
        info[2] = active ? 1 : 0;
        info[3] = !ok ? 1 : (rc == 2 ? 2 : 0);
        if (ok && rc == 2) atomicOr(status, RLVI_ST_NOCONV);
    }
}

// rrm.update_weights on its own: info = { root-find evaluations, 0, 1 if there was a root (0: the alpha -> 0 limit),
// flag }
template <int E>
__global__ __launch_bounds__(SL_THREADS) void moments_rrm_weights_kernel(const double *__restrict__ losses, int n,
                                                                         double eps, double *__restrict__ out,
                                                                         int32_t *__restrict__ info,
                                                                         int32_t *__restrict__ status) {
    extern __shared__ double sm[];
    MoShared sh;
    mo_carve(sh, sm, 0);
    const int tid = threadIdx.x;
    int parity = 0;
    double l[E], w[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        l[j] = losses[q < n ? q : 0];
        w[j] = 0.0;
    }
    // (every thread sees the same eps and n; a loss that is not finite is mo_estep_rrm's to report)
    const bool args = eps > 0.0 && eps < 1.0 && (1.0 - eps) * (double)n > 1.0;
    int evals = 0, rc = 1;
    bool had_root = false;
    if (args) rc = mo_estep_rrm<E, MO_KMAX>(l, w, n, eps, sh.slots, parity, evals, had_root);
    if (rc != 1) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) out[q] = w[j];
        }
    }
    if (tid == 0) {
        info[0] = evals;
        info[1] = 0;
        info[2] = had_root ? 1 : 0;
        info[3] = rc;
        if (rc == 2) atomicOr(status, RLVI_ST_NOCONV);
    }
}

static int mo_check(int64_t n, int64_t d) {
    if (n <= 0 || d <= 0) return RLVI_E_SHAPE;
    return (n >= 2 && n <= SL_MAXN && d <= MO_MAXD && n * d <= MO_MAXND) ? 0 : RLVI_E_LIMIT;
}

// every entry of the six modes: one workgroup, or (BATCH) one per problem of the batch (MODE 3 .. 5: n_eff is eps; no
// estep_tol / estep_maxiter -- the rule is a root, not a fixed point).  theta_init is optional, and checked when given.
template <int MODE, bool BATCH>
static int mo_entry(const double *X, const double *theta_init, int64_t batch, int64_t n, int64_t d,
                    int maxiter, double tol, double etol, int emaxiter, double n_eff, double *theta, double *weights,
                    int32_t *info, void *ws, void *stream) {
    if (const int e = sl_check_args({X, theta, weights, info, ws}, batch, n, d, maxiter >= 0 && emaxiter >= 0,
                                    mo_check(n, d) == 0, {X, theta_init, theta, weights}, {info}, ws))
        return e;
    return sl_moments_form(n, d, [&](auto f) {
        using F = decltype(f);
        return sl_launch(moments_rlvi_kernel<MODE, F::E, F::DS, BATCH>, batch, mo_lds_bytes(n * d),
                         static_cast<hipStream_t>(stream), X, theta_init, (int)n, (int)d, maxiter, tol, etol, emaxiter,
                         n_eff, theta, weights, info, sl_status(ws));
    });
}

// the two weight rules on their own (the slots alone in LDS: no request for more)
template <class GO>
static int mo_weights_entry(const double *losses, int64_t n, bool params_ok, double *out, int32_t *info, void *ws,
                            GO &&go) {
    if (const int e = sl_check_args({losses, out, info, ws}, 1, n, 1, params_ok, n <= SL_MAXN, {losses, out}, {info}, ws))
        return e;
    return sl_samples_per_thread(n, go);
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_moments_check(int64_t n, int64_t d) { return mo_check(n, d); }

extern "C" int rlvi_robust_mean_f64(const double *sample, int64_t n, int64_t d, int maxiter, double tol,
                                    double estep_tol, int estep_maxiter, double *theta, double *weights, int32_t *info,
                                    void *ws, void *stream) {
    return mo_entry<0, false>(sample, nullptr, 1, n, d, maxiter, tol, estep_tol, estep_maxiter, 0.0, theta, weights,
                              info, ws, stream);
}

extern "C" int rlvi_robust_pca_f64(const double *sample, int64_t n, int64_t d, int maxiter, double tol,
                                   const double *theta_init, double estep_tol, int estep_maxiter, double *theta,
                                   double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<1, false>(sample, theta_init, 1, n, d, maxiter, tol, estep_tol, estep_maxiter, 0.0, theta, weights,
                              info, ws, stream);
}

extern "C" int rlvi_robust_covariance_f64(const double *sample, int64_t n, int64_t d, double n_eff, int maxiter,
                                          double tol, double estep_tol, int estep_maxiter, double *theta,
                                          double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<2, false>(sample, nullptr, 1, n, d, maxiter, tol, estep_tol, estep_maxiter, n_eff, theta, weights,
                              info, ws, stream);
}

extern "C" int rlvi_robust_mean_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, int maxiter,
                                          double tol, double estep_tol, int estep_maxiter, double *theta,
                                          double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<0, true>(sample, nullptr, batch, n, d, maxiter, tol, estep_tol, estep_maxiter, 0.0, theta, weights,
                             info, ws, stream);
}

extern "C" int rlvi_robust_pca_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, int maxiter,
                                         double tol, const double *theta_init, double estep_tol, int estep_maxiter,
                                         double *theta, double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<1, true>(sample, theta_init, batch, n, d, maxiter, tol, estep_tol, estep_maxiter, 0.0, theta,
                             weights, info, ws, stream);
}

extern "C" int rlvi_robust_covariance_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double n_eff,
                                                int maxiter, double tol, double estep_tol, int estep_maxiter,
                                                double *theta, double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<2, true>(sample, nullptr, batch, n, d, maxiter, tol, estep_tol, estep_maxiter, n_eff, theta,
                             weights, info, ws, stream);
}

extern "C" int rlvi_update_weights_constrained_f64(const double *losses, int64_t n, double n_eff, double tol,
                                                   int maxiter, double *out, int32_t *info, void *ws, void *stream) {
    return mo_weights_entry(losses, n, maxiter >= 0, out, info, ws, [&](auto f) {
        return sl_launch_plain(moments_uwc_kernel<decltype(f)::E>, 1, mo_lds_bytes(0), static_cast<hipStream_t>(stream),
                               losses, (int)n, n_eff, tol, maxiter, out, info, sl_status(ws));
    });
}

// ---- Robust Risk Minimization
extern "C" int rlvi_rrm_mean_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol,
                                 double *theta, double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<3, false>(sample, nullptr, 1, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_pca_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol,
                                const double *theta_init, double *theta, double *weights, int32_t *info, void *ws,
                                void *stream) {
    return mo_entry<4, false>(sample, theta_init, 1, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_covariance_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol,
                                       double *theta, double *weights, int32_t *info, void *ws, void *stream) {
    return mo_entry<5, false>(sample, nullptr, 1, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_mean_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps,
                                       int maxiter, double tol, double *theta, double *weights, int32_t *info, void *ws,
                                       void *stream) {
    return mo_entry<3, true>(sample, nullptr, batch, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_pca_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps,
                                      int maxiter, double tol, const double *theta_init, double *theta, double *weights,
                                      int32_t *info, void *ws, void *stream) {
    return mo_entry<4, true>(sample, theta_init, batch, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws,
                             stream);
}

extern "C" int rlvi_rrm_covariance_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps,
                                             int maxiter, double tol, double *theta, double *weights, int32_t *info,
                                             void *ws, void *stream) {
    return mo_entry<5, true>(sample, nullptr, batch, n, d, maxiter, tol, 0.0, 0, eps, theta, weights, info, ws, stream);
}

extern "C" int rlvi_rrm_update_weights_f64(const double *losses, int64_t n, double eps, double *out, int32_t *info,
                                           void *ws, void *stream) {
    return mo_weights_entry(losses, n, true, out, info, ws, [&](auto f) {
        return sl_launch_plain(moments_rrm_weights_kernel<decltype(f)::E>, 1, mo_lds_bytes(0),
                               static_cast<hipStream_t>(stream), losses, (int)n, eps, out, info, sl_status(ws));
    });
}
