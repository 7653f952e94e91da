// The weighted least-squares fit of the one-workgroup linear regressions, ONE copy: what linreg_rlvi_kernel
// (standard.hip) and the RRM / Huber regressions (robust_linreg.hip) share.
//   * SlShared (its LDS size is sl_lds_doubles of rlvi_sl_launch.h), the trip sizes SL_XS / SL_RU / SL_GU, the lab
//     stamps (SL_STAMP);
//   * sl_wls: the weighted Gram matrix [X | y]^T W [X | y] on the fp64 matrix cores + the one-wave L D L^T solve with
//     the scale-free pivot test; sl_residuals: the squared residuals and the weighted variance;
//   * sl_ldlt_factor / sl_ldlt_substitute: the one-wave solve split in two, for a system that is factored once and
//     solved for many right-hand sides (Huber's X^T X).
// sl_wls and sl_residuals are linreg_rlvi_kernel's own text, moved here verbatim: that kernel is held to the
// instructions it had (rlvi_sl.h, profiles/r17_sl_header.md).
#pragma once
#include "rlvi_sl.h"

namespace rlvi {

constexpr int SL_XS = 64;                          // 4-row k-panels a wave keeps in registers (resident design: n <= 1024)
constexpr int SL_RU = 4;                           // 16-row blocks of the residual pass in flight per wave and trip
constexpr int SL_GU = 16;                          // 4-row k-panels of the Gram loop in flight per wave and trip

// lab build (-DRLVI_STAMPS=1, tools/build_variants.py): thread 0 leaves 100 MHz wall-clock stamps of the phases in
// the workspace scratch (tools/lab/linreg_phases.py prints them); compiled out of the product library
#if RLVI_STAMPS
#define SL_STAMP() do { if (threadIdx.x == 0 && sh.nst < 120) sh.dbg[sh.nst++] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define SL_STAMP() do { } while (0)
#endif

struct SlShared {
#if RLVI_STAMPS
    mutable unsigned long long *dbg;
    mutable int nst;
#endif
    double *wsh;        // [npad]  weights (pads 0)
    double *rsh;        // [npad]  squared residuals
    double *red;        // [SL_NW][3][256]  Gram partials of the waves
    double *G;          // [SL_DP][SL_GPITCH]
    double *LT;         // [SL_DP][SL_GPITCH]  L^T of the factorisation (row j = column j of L)
    double *th;         // [SL_DP] theta, [SL_DP] previous theta
    double *rhs;        // [SL_DP] X^T W y
    double *slots;      // [2][SL_NW][2]
    int *flag;          // [4]
    double *x1s;        // [1024][8]  columns 16 .. 23 of [X | y] (resident design with two column blocks)
};

// theta = argmin sum_i w_i (y_i - x_i.theta)^2 from the weights in sh.wsh -> sh.th[0 .. d).  Returns false (on
// every thread) when a pivot is not safely positive.  All threads call.  DS: the system is solved padded to DS >= d
// rows -- straight-line code, no guard inside the factorisation; NB: 16-column blocks of [X | y] (2 when d >= 16).
// RES: the design is RESIDENT on the chip (n <= 1024, d <= 23): lane (i, kk) of wave w keeps
// [X | y][4 (w + 4 k) + kk][i], k < 64, in registers (xr) and columns 16 .. 23 live in LDS (sh.x1s) -- no pass over
// global memory after the first.
template <int DS, int NB, bool RES>
__device__ __forceinline__ bool sl_wls(const SlShared &sh, const double *__restrict__ X, const double *__restrict__ y,
                                       int n, int d, const double (&xr)[RES ? SL_XS : 1]) {
    constexpr int DP = NB * 16;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    sd4_t a00 = {0.0, 0.0, 0.0, 0.0}, a01 = a00, a11 = a00;
    const int steps = (n + 3) / 4;
    if constexpr (RES) {
        const int c1 = (i & 7) * 1;
#pragma unroll
        for (int k0 = 0; k0 < SL_XS; k0 += 8) {
            if (4 * (wave + SL_NW * k0) < n) {                        // (wave-uniform: a short design skips its empty blocks)
                double w[8], x1[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;      // < 1024 = the padded length of wsh / x1s
                    w[u] = sh.wsh[row];                              // rows past n: weight 0, panel 0
                    x1[u] = NB > 1 ? sh.x1s[row * 8 + c1] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double x0 = xr[k0 + u];
                    const double w0 = w[u] * x0;
                    a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, x0, a00, 0, 0, 0);
                    if (NB > 1) {
                        const double xb = i < 8 ? x1[u] : 0.0;
                        a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, xb, a01, 0, 0, 0);
                        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(w[u] * xb, xb, a11, 0, 0, 0);
                    }
                }
            }
        }
    } else
    // SL_GU k-panels (4 rows each) per trip, all their loads in flight together: the design comes from the L2
    // (160 KB at n = 1000, d = 20) and a trip's registers are free again before the factorisation needs its own.
    // One CU streams from the L2 at ~45 GB/s (its outstanding misses x the L2's latency), so a pass over the
    // design is microseconds whatever the loop looks like: in-kernel stamps (tools/lab/linreg_phases.py) put this
    // pass and the residual pass at the top of the launch's time beside the E-step's serial reductions.
    for (int s0 = wave; s0 < steps; s0 += SL_GU * SL_NW) {      // (the body of `else` when RES)
        double x0[SL_GU], x1[SL_GU], w[SL_GU];
        int xrow0[SL_GU];
#pragma unroll
        for (int u = 0; u < SL_GU; ++u) {
            const int s = s0 + u * SL_NW;
            const int row = 4 * s + kk;
            const bool ok = s < steps && row < n;
            const int rr = ok ? row : 0;
            // every lane that HAS a column (its column of X, or y) loads from an always valid row, and the value
            // is selected afterwards; the lanes without one (5 of a second block's 16 carry data at d = 20) ask for
            // nothing.  One branch around ALL loads of the trip: a load under a branch of its own is waited for
            // before the next one is issued (the first version of this loop: 64 dependent round trips per trip)
            xrow0[u] = rr;
            w[u] = sh.wsh[rr];
            x0[u] = 0.0;
            x1[u] = 0.0;
        }
        if (i <= d) {
#pragma unroll
            for (int u = 0; u < SL_GU; ++u) x0[u] = *(i < d ? X + (size_t)xrow0[u] * d + i : y + xrow0[u]);
        }
        if (DP > 16 && 16 + i <= d) {
#pragma unroll
            for (int u = 0; u < SL_GU; ++u) x1[u] = *(16 + i < d ? X + (size_t)xrow0[u] * d + 16 + i : y + xrow0[u]);
        }
        __builtin_amdgcn_sched_barrier(0);        // every load of the trip is out before the first value is used
#pragma unroll
        for (int u = 0; u < SL_GU; ++u) {
            // (the predicates again, from the indices: kept across the barrier they are 48 lane masks)
            const int s = s0 + u * SL_NW;
            const bool ok = s < steps && 4 * s + kk < n;
            sl_keep(x0[u]);
            if (DP > 16) sl_keep(x1[u]);
            x0[u] = (ok && i <= d) ? x0[u] : 0.0;
            x1[u] = (DP > 16 && ok && 16 + i <= d) ? x1[u] : 0.0;
            w[u] = ok ? w[u] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < SL_GU; ++u) {
            const double w0 = w[u] * x0[u], w1 = w[u] * x1[u];
            a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, x0[u], a00, 0, 0, 0);
            if (DP > 16) {
                a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, x1[u], a01, 0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(w1, x1[u], a11, 0, 0, 0);
            }
        }
    }
    SL_STAMP();   // gram loop done
    // the waves' partial blocks -> LDS; element e of a block = (result r, lane): row (lane >> 4) + 4 r, column lane & 15
    constexpr int NBLK = NB > 1 ? 3 : 1;
    double *my = sh.red + (size_t)wave * 3 * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        my[0 * 256 + r * 64 + lane] = a00[r];
        if (DP > 16) {
            my[1 * 256 + r * 64 + lane] = a01[r];
            my[2 * 256 + r * 64 + lane] = a11[r];
        }
    }
    __syncthreads();
    // block sums in wave order (deterministic) -> the system PADDED WITH THE IDENTITY to DP rows (a padded row has
    // pivot 1 and no coupling: the factorisation below is straight-line code without a guard), the right-hand
    // side X^T W y (column d) set aside
    for (int e = tid; e < NBLK * 256; e += SL_THREADS) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < SL_NW; ++w) s += sh.red[(size_t)w * 3 * 256 + e];
        const int blk = e >> 8, r = (e >> 6) & 3, l = e & 63;
        const int row = (blk == 2 ? 16 : 0) + (l >> 4) + 4 * r, col = (blk >= 1 ? 16 : 0) + (l & 15);
        const double v = (row < d && col < d) ? s : (row == col ? 1.0 : 0.0);
        sh.G[row * SL_GPITCH + col] = v;
        if (blk == 1) sh.G[col * SL_GPITCH + row] = v;
        if (col == d && row < d) sh.rhs[row] = s;      // (ONE writer per entry: the mirrored element of a diagonal
                                                       //  block is another rounding of the same sum)
    }
    __syncthreads();
    SL_STAMP();   // block sums done
    // ---- wave 0: G = L D L^T, row t of the lower triangle in lane t's registers
    // (sl_ldlt_solve<DS> of rlvi_sl.h in place: the call moves this kernel's register allocation, and with it single
    //  cells of tools/lab/sweep_linreg.py by up to 2 % either way -- profiles/r17_sl_header.md)
    if (wave == 0) {
        int t = lane & (SL_DP - 1);
        // (opaque: the lane masks t > j, t == j below are loop-invariant across the estimator's outer loop, and
        //  hoisted there they are 2 DP scalar register pairs that spill)
        asm volatile("" : "+v"(t));
        double g[DS];
#pragma unroll
        for (int c = 0; c < DS; ++c) g[c] = sh.G[t * SL_GPITCH + c];
        double b = t < d ? sh.rhs[t < SL_DP ? t : 0] : 0.0;
        double dinv = 0.0;                       // lane j: 1 / D_j
#pragma unroll
        for (int j = 0; j < DS; ++j) {
            const double piv = sl_readlane(g[j], j);
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
            sh.LT[j * SL_GPITCH + t] = g[j];                          // row j of L^T: for the back substitution
            __builtin_amdgcn_sched_barrier(0);
        }
        // L z = b (lane t ends with z_t; g[j] = 0 for t <= j: no mask), then z / D
#pragma unroll
        for (int j = 0; j < DS; ++j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
        b *= dinv;
        // L^T theta = z: lane t needs column t of L = row t of L^T (0 for c <= t: no mask)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int c = 0; c < DS; ++c) g[c] = sh.LT[t * SL_GPITCH + c];
#pragma unroll
        for (int j = DS - 1; j >= 1; --j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
        if (lane < d) sh.th[lane] = b;
        // The pivot test, behind the solve: lane t's own pivot against lane t's own diagonal entry, D_t > G_tt d 64 eps.
        // D_t / G_tt is 1 - R^2 of column t regressed on the columns before it -- it does not move when a column is
        // rescaled, so a column of 1e-8 or a timestamp of 1e9 beside unit features is not read as rank deficiency
        // (against the LARGEST diagonal entry it was, and the general path then dropped the column: DESIGN 3.4b).
        // Lane t still holds 1 / D_t and G is untouched in LDS: the test is floor_t / D_t < 1 with a positive, finite
        // 1 / D_t (a pivot of 0, inf or NaN leaves a NaN there), nothing of it is live across the factorisation (a
        // pivot or a floor kept in registers through the loop spills: profiles/r22_linreg_designs.md) and the lanes'
        // verdicts are combined once -- no broadcast per pivot.
        const double gtt = t < d ? sh.G[t * SL_GPITCH + t] : 0.0;
        const double dmax = wave_max(gtt);
        const bool bad = !(dmax == dmax) || __any(t < d && !(dinv > 0.0 && sl_pivot_floor(gtt, d) * dinv < 1.0));
        if (lane == 0) sh.flag[0] = bad ? 1 : 0;
    }
    __syncthreads();
    SL_STAMP();   // solved
    return sh.flag[0] == 0;
}

// r_i = (y_i - x_i.theta)^2 -> sh.rsh, sigma2 = w.r / sum(w); returns sigma2 on every thread
template <int NB, bool RES>
__device__ __forceinline__ double sl_residuals(const SlShared &sh, const double *__restrict__ X,
                                               const double *__restrict__ y, int n, int d, int &parity,
                                               const double (&xr)[RES ? SL_XS : 1]) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int i = lane & 15, kk = lane >> 4;
    double num = 0.0, den = 0.0;
    if constexpr (RES) {
        // from the resident panels: lane (i, kk) holds [X | y][row][i] (and reads [row][16 + i], i < 8, from LDS); with
        // c = [theta; -1 in column d] the row's x.theta - y is the sum over the 16 lanes of a row's group -- four
        // DPP steps -- and its square is the residual.  No matrix instruction (they contract over the ROWS of a
        // panel, which is the Gram matrix's sum), no byte from global memory.
        const double c0 = i < d ? sh.th[i] : (i == d ? -1.0 : 0.0);
        const int j1 = 16 + (i & 7);
        const double c1 = (NB > 1 && i < 8) ? (j1 < d ? sh.th[j1 < SL_DP ? j1 : 0] : (j1 == d ? -1.0 : 0.0)) : 0.0;
#pragma unroll
        for (int k0 = 0; k0 < SL_XS; k0 += 8) {
            // eight panels per block of straight-line code (their LDS reads and butterflies interleave); a short
            // design skips its empty blocks (wave-uniform)
            if (4 * (wave + SL_NW * k0) < n) {
                double p[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;
                    p[u] = xr[k0 + u] * c0;
                    if (NB > 1) p[u] = __builtin_fma(sh.x1s[row * 8 + (i & 7)], c1, p[u]);
                }
                // the eight partials of a lane -> the eight row sums of its 16-lane group, TRANSPOSING on the way:
                // after the exchange with lane ^ 1 a lane keeps the panels of its own parity (four values), after
                // lane ^ 2 two, and those two are finished by two rotations of the row -- 54 cross-lane instructions for
                // eight panels instead of 96; lane (b2 b1) of a group ends with the sums of panels b2b1 and 4 + b2b1
                const bool b1 = (i & 1) != 0, b2 = (i & 2) != 0;
                double q[4], r[2];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const double keep = b1 ? p[2 * m + 1] : p[2 * m], send = b1 ? p[2 * m] : p[2 * m + 1];
                    q[m] = keep + dpp_x<0xB1>(send);                 // quad_perm [1,0,3,2]
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const double keep = b2 ? q[2 * m + 1] : q[2 * m], send = b2 ? q[2 * m] : q[2 * m + 1];
                    r[m] = keep + dpp_x<0x4E>(send);                 // quad_perm [2,3,0,1]
                    // (the partners of the last two steps must share the lane's low two bits: rotations by 8 and by 4
                    //  inside the 16-lane row, not the mirrors)
                    r[m] = r[m] + dpp_x<0x128>(r[m]);                // row_ror:8
                    r[m] = r[m] + dpp_x<0x124>(r[m]);                // row_ror:4
                }
                // lanes 0 .. 3 of a group keep the sums and write the residuals of panels i and 4 + i
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int u = 4 * m + (i & 3);
                    const int row = 4 * (wave + SL_NW * (k0 + u)) + kk;
                    const double rr = r[m] * r[m];
                    const double wr = i < 4 ? sh.wsh[row] : 0.0;
                    if (i < 4) sh.rsh[row] = rr;
                    num = __builtin_fma(wr, rr, num);
                    den += wr;
                }
            }
        }
        sl_block_sum2(num, den, sh.slots, parity);
        SL_STAMP();   // residuals done
        return num / den;
    }
    const int blocks = (n + 15) / 16;
    // X[16 rb .. +15] . theta on the matrix cores: A = a 16 x 4 panel of X, B = the 4 matching entries of theta in
    // every column; lane l's results are rows (l >> 4) + 4 r, all columns alike.  SL_RU row blocks per wave and
    // trip, all their loads in flight together (one block per trip was one L2 round trip per 16 rows: 11 us per
    // pass at n = 1000).
    double bv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {                                    // d <= 31: eight 4-column panels at most
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
            const int r = 16 * rb + kk + 4 * i;
            if (i < 4 && r < n) {
                const double p = i == 0 ? acc[0] : i == 1 ? acc[1] : i == 2 ? acc[2] : acc[3];
                const double e = yv[q] - p, rr = e * e;
                const double w = sh.wsh[r];
                sh.rsh[r] = rr;
                num = __builtin_fma(w, rr, num);
                den += w;
            }
        }
    }
    sl_block_sum2(num, den, sh.slots, parity);      // (its barrier also publishes rsh)
    SL_STAMP();   // residuals done
    return num / den;
}

// ---- the one-wave solve of sl_wls in two parts, for a system that is factored ONCE and solved for many right-hand
// sides (Huber's X^T X: the design never changes).  sl_wls keeps its own solve in place (see there).
//
// ONE WAVE: G = L D L^T for the symmetric G [SL_DP][SL_GPITCH] in LDS, padded with the identity beyond its d rows and
// factored as DS >= d rows.  Left behind in LDS: LT [SL_DP][SL_GPITCH] (row j = column j of L, strictly lower part, 0
// elsewhere; rows j < DS) and dinv [SL_DP] (1 / D_t; 0 for t >= DS).  *flag: 1 when a pivot is not safely positive by
// the scale-free test of sl_wls (D_t against G_tt d 64 eps), or not a number.  The caller puts a workgroup barrier
// behind the call before another wave reads any of it.
template <int DS>
__device__ __forceinline__ void sl_ldlt_factor(const double *G, double *LT, int d, double *dinv_out, int *flag) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int t = lane & (SL_DP - 1);
    double g[DS];
#pragma unroll
    for (int c = 0; c < DS; ++c) g[c] = G[t * SL_GPITCH + c];
    double dinv = 0.0;                       // lane j: 1 / D_j
#pragma unroll
    for (int j = 0; j < DS; ++j) {
        const double piv = sl_readlane(g[j], j);
        const double inv = sl_rcp(piv);
        const double l = g[j] * inv;                              // L[t][j] for t > j
        dinv = t == j ? inv : dinv;
#pragma unroll
        for (int c = j + 1; c < DS; ++c) {
            const double lc = sl_readlane(g[j], c);              // G[c][j] = L[c][j] D_j
            g[c] = __builtin_fma(-l, lc, g[c]);                  // (lanes t < c compute values nobody reads)
            if (((c - j) & 7) == 0) __builtin_amdgcn_sched_barrier(0);
        }
        g[j] = t > j ? l : 0.0;
        LT[j * SL_GPITCH + t] = g[j];
        __builtin_amdgcn_sched_barrier(0);
    }
    if (lane < SL_DP) dinv_out[lane] = dinv;
    const double gtt = t < d ? G[t * SL_GPITCH + t] : 0.0;
    const double dmax = wave_max(gtt);
    const bool bad = !(dmax == dmax) || __any(t < d && !(dinv > 0.0 && sl_pivot_floor(gtt, d) * dinv < 1.0));
    if (lane == 0) flag[0] = bad ? 1 : 0;
}

// ONE WAVE: x = G^-1 rhs from what sl_ldlt_factor<DS> left in LT and dinv: L z = rhs, z / D, L^T x = z, a row per lane
// and v_readlane broadcasts.  rhs [d] and x [d] are in LDS (they may be the same array); LT, dinv and rhs may have
// been written by this wave just before.  The caller puts a workgroup barrier behind the call.
template <int DS>
__device__ __forceinline__ void sl_ldlt_substitute(const double *LT, const double *dinv, const double *rhs, int d,
                                                   double *x) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int t = lane & (SL_DP - 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double g[DS];
#pragma unroll
    for (int j = 0; j < DS; ++j) g[j] = LT[j * SL_GPITCH + t];   // row t of L (0 for j >= t: no mask below)
    double b = t < d ? rhs[t] : 0.0;
#pragma unroll
    for (int j = 0; j < DS; ++j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
    b *= dinv[t];
#pragma unroll
    for (int c = 0; c < DS; ++c) g[c] = LT[t * SL_GPITCH + c];   // column t of L = row t of L^T (0 for c <= t)
#pragma unroll
    for (int j = DS - 1; j >= 1; --j) b = __builtin_fma(-g[j], sl_readlane(b, j), b);
    if (lane < d) x[lane] = b;
}

}  // namespace rlvi
