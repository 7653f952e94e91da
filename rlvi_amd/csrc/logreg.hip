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
#include "rlvi_sl.h"

namespace rlvi {

constexpr int LG_RU = 4;                           // 16-row blocks of Z.v in flight per wave and trip
constexpr int LG_GU = 16;                          // 4-row k-panels of the Gram loop in flight per wave and trip
constexpr int LG_MAXD = SL_DP - 2;                 // [X | 1] and the gradient's column in two 16-column blocks
constexpr int LG_NEWTON_CAP = 50;                  // Newton steps of one fit
constexpr int LG_HALVINGS = 40;                    // Armijo trials of one step
constexpr double LG_GTOL2 = 1e-24;                 // (1e-12)^2: ||g|| <= 1e-12 ||g(0)||
constexpr double LG_ARMIJO = 1e-4;
// the rounding floor: f is flat to second order, so below g.delta <= LG_FLOOR |f| its sums cannot tell a good step
// from a bad one.  A full step that Armijo refuses there, but that changes f by no more than LG_NOISE |f|, is taken on
// the gradient's word; the fit ends when the next gradient has not shrunk to half (a quarter of its square).
constexpr double LG_FLOOR = 1e-10;
constexpr double LG_NOISE = 1e-12;

// lab build (-DRLVI_STAMPS=1): thread 0 leaves 100 MHz wall-clock stamps of the phases at the start of the workspace
// scratch (tools/lab/logreg_phases.py prints them; one stamp scheme per run, rlvi_stamps.h); compiled out otherwise
#if RLVI_STAMPS
#define LG_STAMP(code) do { if (threadIdx.x == 0 && sh.nst < 480) { sh.dbg[sh.nst++] = __builtin_amdgcn_s_memrealtime(); \
                                                                   sh.dbg[sh.nst++] = (code); } } while (0)
#else
#define LG_STAMP(code) do { } while (0)
#endif

struct LgShared : SlSolve {      // th: v = (coef, bias), rhs: Z^T (C what s p)
#if RLVI_STAMPS
    mutable unsigned long long *dbg;
    mutable int nst;
#endif
    double *zsh;        // [npad]  z = X coef + bias
    double *hsh;        // [npad]  C what p (1 - p): the Hessian's coefficient
    double *csh;        // [npad]  C what s p: the gradient's coefficient; behind the Gram pass: Z.delta
    double *gv;         // [SL_DP] the gradient
    double *dl;         // [SL_DP] the Newton direction
};

// logreg_rlvi_kernel's LDS in doubles: zsh, hsh, csh, gv, dl, then the solve's block
__host__ __device__ constexpr size_t lg_solve_off(int npad) { return 3 * (size_t)npad + 2 * SL_DP; }
__host__ __device__ constexpr size_t lg_lds_doubles(int npad) { return lg_solve_off(npad) + SL_SOLVE_DOUBLES; }

// log(1 + exp(-m)), overflow-safe; em = exp(-|m|)
__device__ __forceinline__ double lg_softplus_neg(double m, double em) {
    return log1p(em) + (m < 0.0 ? -m : 0.0);
}

// G = I + Z^T diag(h) Z ([X | 1]: D = d + 1 rows, padded with the identity to SL_DP) and rhs = Z^T c from hsh / csh.
// The loop of sl_wls (standard.hip): LG_GU k-panels of 4 rows per wave and trip with all their loads in flight
// together; the left factor is the panel of [X | 1], the right one h times it with c in column D.  All threads call;
// ends with a barrier.
template <int NB>
__device__ __forceinline__ void lg_gram(const LgShared &sh, const double *__restrict__ X, int n, int d) {
    constexpr int DP = NB * 16;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    const int D = d + 1;
    sd4_t a00 = {0.0, 0.0, 0.0, 0.0}, a01 = a00, a11 = a00;
    const int steps = (n + 3) / 4;
    for (int s0 = wave; s0 < steps; s0 += LG_GU * SL_NW) {
        double x0[LG_GU], x1[LG_GU], h[LG_GU], c[LG_GU];
        int xrow0[LG_GU];
#pragma unroll
        for (int u = 0; u < LG_GU; ++u) {
            const int s = s0 + u * SL_NW;
            const int row = 4 * s + kk;
            const bool ok = s < steps && row < n;
            const int rr = ok ? row : 0;                 // (always a valid row; selected away below)
            xrow0[u] = rr;
            h[u] = sh.hsh[rr];
            c[u] = sh.csh[rr];
            x0[u] = 1.0;                                 // column d of [X | 1]
            x1[u] = 1.0;
        }
        // one branch around ALL loads of a block's columns: a load under a branch of its own is waited for before the
        // next one is issued
        if (i < d) {
#pragma unroll
            for (int u = 0; u < LG_GU; ++u) x0[u] = X[(size_t)xrow0[u] * d + i];
        }
        if (DP > 16 && 16 + i < d) {
#pragma unroll
            for (int u = 0; u < LG_GU; ++u) x1[u] = X[(size_t)xrow0[u] * d + 16 + i];
        }
        __builtin_amdgcn_sched_barrier(0);        // every load of the trip is out before the first value is used
#pragma unroll
        for (int u = 0; u < LG_GU; ++u) {
            const int s = s0 + u * SL_NW;
            const bool ok = s < steps && 4 * s + kk < n;
            sl_keep(x0[u]);
            if (DP > 16) sl_keep(x1[u]);
            x0[u] = (ok && i < D) ? x0[u] : 0.0;
            x1[u] = (DP > 16 && ok && 16 + i < D) ? x1[u] : 0.0;
            h[u] = ok ? h[u] : 0.0;
            c[u] = ok ? c[u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < LG_GU; ++u) {
            // right factor: h x in the columns of [X | 1], c in column D (the left factor is 0 there)
            const double b0 = i == D ? c[u] : h[u] * x0[u];
            a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], b0, a00, 0, 0, 0);
            if (DP > 16) {
                const double b1 = 16 + i == D ? c[u] : h[u] * x1[u];
                a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[u], b1, a01, 0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], b1, a11, 0, 0, 0);
            }
        }
    }
    // the waves' partial blocks -> I + the Gram matrix, the gradient's part Z^T c (column D) set aside
    sl_gram_collect<NB, true>(sh, D, a00, a01, a11);
}

// out[r] = x_r . vec[0 .. d) + vec[d] for the rows r < n: 16 rows per wave and instruction on the matrix cores (the
// residual pass of standard.hip), LG_RU row blocks per wave and trip with their loads in flight together.  The
// caller puts a barrier behind it.
__device__ __forceinline__ void lg_matvec(const double *__restrict__ X, int n, int d, const double *vec, double *out) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    const int blocks = (n + 15) / 16;
    const double bias = vec[d];
    double bv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {                                    // d <= 30: eight 4-column panels at most
        const int k = 4 * u + kk;
        const double tv = vec[k < d ? k : 0];
        bv[u] = k < d ? tv : 0.0;
    }
    for (int rb0 = wave; rb0 < blocks; rb0 += LG_RU * SL_NW) {
        double a[LG_RU][8];
#pragma unroll
        for (int q = 0; q < LG_RU; ++q) {
            const int rb = rb0 + q * SL_NW;
            const int row = 16 * rb + i;
            const double *xrow = X + (size_t)(row < n ? row : 0) * d;
#pragma unroll
            for (int u = 0; u < 8; ++u) a[q][u] = xrow[(4 * u + kk) < d ? 4 * u + kk : 0];      // (branch-free)
        }
        __builtin_amdgcn_sched_barrier(0);        // every load of the trip is out before the first value is used
#pragma unroll
        for (int q = 0; q < LG_RU; ++q) {
            const int rb = rb0 + q * SL_NW;
            const bool rok = 16 * rb + i < n;
            sd4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                sl_keep(a[q][u]);
                const double av = (rok && 4 * u + kk < d) ? a[q][u] : 0.0;
                if (4 * u < d) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[u], acc, 0, 0, 0);
            }
            const int r = 16 * rb + kk + 4 * i;
            if (i < 4 && r < n) out[r] = (i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3]) + bias;
        }
    }
}

// v = argmin 1/2 v.v + sum_i cw_i log(1 + exp(-s_i z_i)) by damped Newton from v = 0; sgn[j] = s and cw[j] = C what of
// this thread's sample tid + 256 j (cw = 0 past n).  Leaves v in sh.th[0 .. d], z = Z v (one fresh pass) in sh.zsh, adds
// its Newton steps to `newton`.  Returns, on every thread, 0, 1 (not finite, or a pivot not safely positive) or
// 2 (LG_NEWTON_CAP steps without reaching the stop test, or LG_HALVINGS Armijo trials away from the rounding floor
// without an acceptable step: the result is the last accepted point).  All threads call.
template <int E, int DS, int NB>
__device__ __forceinline__ int lg_fit(const LgShared &sh, const double *__restrict__ X, int n, int d,
                                      const double (&sgn)[E], const double (&cw)[E], int &parity, int &newton) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int D = d + 1;
    if (tid < SL_DP) sh.th[tid] = 0.0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int q = tid + j * SL_THREADS;
        if (q < n) sh.zsh[q] = 0.0;
    }
    __syncthreads();
    double g0 = 0.0, gg_noise = -1.0;
    int rc = 0;
    for (int step = 0;; ++step) {
        LG_STAMP(1);   // Newton step starts
        // ---- p = sigma(-s z), f and the two coefficients, on the thread's own samples
        double fs = 0.0, none = 0.0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            const bool v = q < n;
            const double z = sh.zsh[v ? q : 0];
            const double m = sgn[j] * z;
            const double em = exp(-fabs(m));
            const double r = 1.0 / (1.0 + em);
            const double p = m >= 0.0 ? em * r : r, q1 = m >= 0.0 ? r : em * r;    // sigma(-m), 1 - sigma(-m)
            if (v) {
                fs = __builtin_fma(cw[j], lg_softplus_neg(m, em), fs);
                sh.csh[q] = sgn[j] * cw[j] * p;
                sh.hsh[q] = cw[j] * p * q1;
            }
        }
        sl_block_sum2(fs, none, sh.slots, parity);                  // (its barrier publishes csh / hsh)
        const double vl = lane < D ? sh.th[lane] : 0.0;
        const double f = 0.5 * wave_sum(vl * vl) + fs;
        if (!(f < __builtin_inf())) { rc = 1; break; }
        LG_STAMP(2);   // objective done
        lg_gram<NB>(sh, X, n, d);
        LG_STAMP(3);   // Gram matrix done
        const double gl = lane < D ? vl - sh.rhs[lane] : 0.0;         // g = v - Z^T (C what s p)
        const double gg = wave_sum(gl * gl);
        if (step == 0) g0 = gg;
        if (!(gg < __builtin_inf())) { rc = 1; break; }
        if (gg <= LG_GTOL2 * g0) break;
        if (gg_noise >= 0.0 && !(gg <= 0.25 * gg_noise)) break;      // the floor: the gradient no longer shrinks
        gg_noise = -1.0;
        if (step >= LG_NEWTON_CAP) { rc = 2; break; }
        if (tid < SL_DP) sh.gv[tid] = gl;
        __syncthreads();
        if (wave == 0) sl_ldlt_solve<DS>(sh.G, sh.LT, sh.gv, D, sh.dl, sh.flag);
        __syncthreads();
        ++newton;
        if (sh.flag[0] != 0) { rc = 1; break; }
        LG_STAMP(4);   // solved
        const double dv = lane < D ? sh.dl[lane] : 0.0;
        const double gd = wave_sum(gl * dv);
        lg_matvec(X, n, d, sh.dl, sh.csh);                          // Z.delta (csh is free behind the Gram pass)
        __syncthreads();
        LG_STAMP(5);   // Z.delta done
        // ---- Armijo: the largest t = 2^-k with f(v - t delta) <= f(v) - 1e-4 t g.delta
        double t = 1.0;
        bool accepted = false, at_floor = false;
        for (int k = 0; k < LG_HALVINGS; ++k) {
            double ft = 0.0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                const bool v = q < n;
                const double z = sh.zsh[v ? q : 0] - t * sh.csh[v ? q : 0];
                const double m = sgn[j] * z;
                const double l = lg_softplus_neg(m, exp(-fabs(m)));
                if (v) ft = __builtin_fma(cw[j], l, ft);
            }
            sl_block_sum2(ft, none, sh.slots, parity);
            const double vt = vl - t * dv;
            ft += 0.5 * wave_sum(vt * vt);
            if (ft <= f - LG_ARMIJO * t * gd) { accepted = true; break; }
            if (k == 0 && gd <= LG_FLOOR * fabs(f)) {                // the floor (LG_FLOOR above)
                at_floor = true;
                if (ft <= f + LG_NOISE * fabs(f)) { accepted = true; gg_noise = gg; }
                break;
            }
            t *= 0.5;
        }
        LG_STAMP(6);   // line search done
        if (!accepted) {
            if (!at_floor) rc = 2;                                   // no step at all: never a silent "converged"
            break;
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int q = tid + j * SL_THREADS;
            if (q < n) sh.zsh[q] -= t * sh.csh[q];
        }
        if (tid < D) sh.th[tid] = vl - t * dv;                       // (wave 0: lane == tid)
        __syncthreads();
    }
    if (rc == 1) return rc;
    __syncthreads();
    lg_matvec(X, n, d, sh.th, sh.zsh);                              // z of the result, not of the steps' sum
    __syncthreads();
    LG_STAMP(7);   // fit done
    return rc;
}

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

// one workgroup, or (BATCH) one per problem of the batch: ONE dispatch rule for both forms
template <bool BATCH = false>
static int lg_launch(const double *X, const double *y, const double *w_in, int64_t n, int64_t d, int mode,
                     int maxiter, double tol, double etol, int emaxiter, double creg, double *theta, double *w_out,
                     double *losses, int32_t *info, void *ws, hipStream_t st, int64_t batch = 1) {
    const int npad = (int)((n + 63) / 64) * 64;
    const size_t lds = lg_lds_doubles(npad) * sizeof(double);
    int32_t *status = &static_cast<WsHeader *>(ws)->status;
    auto go = [&](auto kern) {
        // (asked for per kernel: allow_dyn_lds keeps its once-per-device state by the kernel's address)
        if (const int e = allow_dyn_lds(kern, 150 * 1024)) return e;
        return launch(kern, dim3(BATCH ? (unsigned)batch : 1u), dim3(SL_THREADS), lds, st, X, y, w_in, (int)n, (int)d,
                      npad, mode, maxiter, tol, etol, emaxiter, creg, theta, w_out, losses, info, status,
                      stamp_base(ws));
    };
    // samples per thread (1 / 4 / 16); the system of d + 1 unknowns solved padded to 4 / 16 / 24 / 32 rows; [X | 1]
    // and the gradient's column in one 16-column block (d <= 14) or two
#define RLVI_LG(E_)                                                     \
    do {                                                                \
        if (d <= 3) return go(logreg_rlvi_kernel<E_, 4, 1, BATCH>);     \
        if (d <= 14) return go(logreg_rlvi_kernel<E_, 16, 1, BATCH>);   \
        if (d <= 23) return go(logreg_rlvi_kernel<E_, 24, 2, BATCH>);   \
        return go(logreg_rlvi_kernel<E_, 32, 2, BATCH>);                \
    } while (0)
    if (n <= SL_THREADS) RLVI_LG(1);
    if (n <= 4 * SL_THREADS) RLVI_LG(4);
    RLVI_LG(16);
#undef RLVI_LG
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_logistic_regression_check(int64_t n, int64_t d) { return lg_check(n, d); }

extern "C" int rlvi_logistic_regression_f64(const double *X, const double *y, int64_t n, int64_t d, int maxiter,
                                            double tol, double estep_tol, int estep_maxiter, double C, double *theta,
                                            double *weights, double *losses, int32_t *info, void *ws, void *stream) {
    if (sl_any_null({X, y, theta, weights, info, ws})) return RLVI_E_NULL;
    if (n <= 0 || d <= 0 || maxiter < 0 || estep_maxiter < 0 || !(C > 0.0)) return RLVI_E_SHAPE;
    if (lg_check(n, d)) return RLVI_E_LIMIT;
    if (sl_misaligned({X, y, theta, weights, losses}, info, ws)) return RLVI_E_ALIGN;
    return lg_launch<>(X, y, nullptr, n, d, 0, maxiter, tol, estep_tol, estep_maxiter, C, theta, weights, losses, info,
                     ws, static_cast<hipStream_t>(stream));
}

extern "C" int rlvi_logistic_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                                  int maxiter, double tol, double estep_tol, int estep_maxiter,
                                                  double C, double *theta, double *weights, double *losses,
                                                  int32_t *info, void *ws, void *stream) {
    if (sl_any_null({X, y, theta, weights, info, ws})) return RLVI_E_NULL;
    if (batch <= 0 || n <= 0 || d <= 0 || maxiter < 0 || estep_maxiter < 0 || !(C > 0.0)) return RLVI_E_SHAPE;
    if (batch > SL_MAXBATCH || lg_check(n, d)) return RLVI_E_LIMIT;
    if (sl_misaligned({X, y, theta, weights, losses}, info, ws)) return RLVI_E_ALIGN;
    return lg_launch<true>(X, y, nullptr, n, d, 0, maxiter, tol, estep_tol, estep_maxiter, C, theta, weights, losses,
                           info, ws, static_cast<hipStream_t>(stream), batch);
}

extern "C" int rlvi_logistic_fit_f64(const double *X, const double *y, const double *w, int64_t n, int64_t d, double C,
                                     double *theta, double *losses, int32_t *info, void *ws, void *stream) {
    if (sl_any_null({X, y, w, theta, losses, info, ws})) return RLVI_E_NULL;
    if (n <= 0 || d <= 0 || !(C > 0.0)) return RLVI_E_SHAPE;
    if (lg_check(n, d)) return RLVI_E_LIMIT;
    if (sl_misaligned({X, y, w, theta, losses}, info, ws)) return RLVI_E_ALIGN;
    return lg_launch<>(X, y, w, n, d, 1, 0, 0.0, 0.0, 0, C, theta, nullptr, losses, info, ws,
                     static_cast<hipStream_t>(stream));
}
