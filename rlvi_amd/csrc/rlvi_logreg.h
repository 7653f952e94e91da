// The weighted logistic fit of the one-workgroup estimators, ONE copy: logreg_rlvi_kernel (logreg.hip: RLVI's
// logistic regression, the fit on its own) and logreg_rrm_kernel (robust_logreg.hip: RRM's) call it.  The text is
// logreg.hip's, moved verbatim: the constants, LgShared and its LDS sizes, lg_softplus_neg, lg_gram, lg_matvec, lg_fit.
#pragma once
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

}  // namespace rlvi
