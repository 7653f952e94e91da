// The online path's mini-batch as ONE launch, and a whole stream of them as one.
//
//   rlvi_online_step_f64     online-learning/main.py:291-313, :318-331   residuals -> sample weights -> partial_fit ->
//                                                                        the four test counts, for one classifier
//   rlvi_online_stream_f64   main.py:288-339                             T mini-batches for S classifiers
//
// partial_fit is scikit-learn's `_plain_sgd` with the reference's settings (SGDClassifier(loss='log_loss',
// random_state=1): L2 penalty, learning rate 'optimal', an intercept, one shuffled epoch, no averaging): a recurrence
// over the samples, each step a dot product of d <= 128 numbers, one exp and two divisions.  Nothing in it is parallel
// but the dot product, so ONE wave owns it: lane l holds columns l and l + 64 of the weight vector in registers, the dot
// product is a lane product and the wave's butterfly sum (no LDS, no barrier), and the scalars of the step (wscale,
// intercept, t) are the same in every lane.  The order of the pass is an input (a few integers the host computes: it
// depends on n alone), so nothing the recurrence waits for is a load: before the pass all four waves lay out what it
// reads IN PASS ORDER in LDS (row index, label, sample weight), and the wave fetches the rows of eight samples
// while it steps through the eight before them.
// Around the pass, all four waves: the residuals -log sigmoid(x.coef + intercept) (a wave per row, the same lane
// product and butterfly as the pass), the weights (update_weights_rlvi with the arithmetic of online_weight_kernel,
// standard.hip, or RRM's rule of rlvi_rrm.h) on the threads' own samples, and the decision values of the test rows with
// the new state, counted into (tp, tn, fp, fn).
// The stream form is the same code in a loop over the batches, one workgroup per classifier, the state kept in LDS
// between batches: a (classifier, batch) has the bits of the same sequence of single steps.
// Sums are fp64 in a fixed order: same inputs, same bits.
#include <math.h>

#include "rlvi_rrm.h"
#include "rlvi_sl_launch.h"

namespace rlvi {

constexpr int ON_MAXD = 128;                       // two columns per lane
constexpr int ON_MAXS = 8;                         // classifiers of one stream launch
constexpr int64_t ON_MAXT = 1 << 20;               // batches of one stream launch
constexpr int ON_STATE = ON_MAXD + 8;              // LDS doubles of the state (coef [d], intercept, t)
constexpr int ON_STRIDE = 3;                       // the slot stride (mo_estep_rrm sums three values)
constexpr int ON_CH = 8;                           // samples whose rows are fetched together
constexpr double ON_MAX_DLOSS = 1e12;

struct OnArgs {
    const double *X, *y, *Xt, *yt;                 // [T, n, d], [T, n], [T, m, d], [T, m]
    const int32_t *rows, *orders;                  // [T, 2] or NULL (every batch n and m rows), [T, n] or NULL (natural)
    const double *state_in;                        // [d + 2], read unless first
    double *state_out;                             // [S, T, d + 2]
    double *weights;                               // [S, T, n] or NULL (read where a classifier's method is 3)
    int32_t *counts, *info;                        // [S, T, 4] each
    int T, n, m, d, npad, first, maxiter;
    double alpha, oinit, tol;
    int method[ON_MAXS];
    double eps[ON_MAXS];
};

// this lane's two products of a row with a vector held two columns per lane, summed over the wave.  x0, x1: 0 in a lane
// whose column is past d.
__device__ __forceinline__ double on_dot(double x0, double x1, double c0, double c1) {
    return wave_sum(__builtin_fma(x1, c1, x0 * c0));
}

// update_weights_rlvi (main.py:45-58) on this thread's samples tid + 256 j: the arithmetic of online_weight_kernel
// (standard.hip), same bits for the same residuals.  Returns the iterations.
template <int E>
__device__ __forceinline__ int on_estep_rlvi(const double (&l)[E], double (&w)[E], int n, double tol, int maxiter,
                                             double *slots, int &parity) {
    const int tid = threadIdx.x;
    double e[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const bool v = tid + j * SL_THREADS < n;
        e[j] = v ? exp(-l[j]) : 0.0;                                // main.py:47
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
        sl_block_sum2<ON_STRIDE>(sse, sum, slots, parity);
        ++it;
        if (sqrt(sse) < tol) break;                                 // main.py:53-56
        const double avg = sum * invn;                              // main.py:50-51
        ratio = avg / (1.0 - avg);
    }
    double mx = -__builtin_inf();                                   // new /= max(new) * len(new) (main.py:57)
#pragma unroll
    for (int j = 0; j < E; ++j)
        if (tid + j * SL_THREADS < n) mx = w[j] > mx ? w[j] : mx;
    mx = sl_block_max<ON_STRIDE>(mx, slots, parity);
    const double den = mx * (double)n;
#pragma unroll
    for (int j = 0; j < E; ++j) w[j] = w[j] / den;
    return it;
}

// info of a (classifier, batch) = { E-step iterations (RLVI) or root-find evaluations (RRM), 1 if RRM had a root, samples
// whose update was not zero, flag }.  flag 1: a coefficient or the intercept is not finite (scikit-learn raises
// ValueError there; the state is written as it is); 2: no weights (a residual not finite, or RRM's eps with (1 - eps) n
// <= 1): no pass, the state as it was; 3: RRM's root-find at its 200 evaluations (results written); 4: a row count or
// an index of the order out of range: nothing read through it, no pass.
template <int E>
__global__ __launch_bounds__(SL_THREADS) void online_sgd_kernel(OnArgs a) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int s = blockIdx.x, d = a.d, npad = a.npad;
    double *const csh = sm;
    double *const slots = csh + ON_STATE;
    double *const lsh = slots + sl_slot_doubles(ON_STRIDE);        // residuals, then the weights, by sample
    double *const cy = lsh + npad;                                  // in pass order: label (1 or 0) 
    double *const csw = cy + npad;                                  //                sample weight
    int *const cidx = reinterpret_cast<int *>(csw + npad);         //                row
    int *const cnt = cidx + npad;                                   // [4] counts, [2] the pass's flag and updates
    int parity = 0;
    int method = a.method[0];                                       // (selects, not an indexed read of the arguments)
    double eps = a.eps[0];
#pragma unroll
    for (int k = 1; k < ON_MAXS; ++k) {
        method = s == k ? a.method[k] : method;
        eps = s == k ? a.eps[k] : eps;
    }
    const bool k0 = lane < d, k1 = lane + WAVE < d;
    const int o0 = k0 ? lane : 0, o1 = k1 ? lane + WAVE : 0;

    if (tid < d + 2) csh[tid] = a.first ? (tid == d + 1 ? 1.0 : 0.0) : a.state_in[tid];     // unfitted: t = 1
    __syncthreads();

    for (int t = 0; t < a.T; ++t) {
        const int nt = a.rows ? a.rows[2 * t] : a.n, mt = a.rows ? a.rows[2 * t + 1] : a.m;
        const size_t st = (size_t)s * a.T + t;
        const double *X = a.X + (size_t)t * a.n * d, *y = a.y + (size_t)t * a.n;
        const int32_t *ord = a.orders ? a.orders + (size_t)t * a.n : nullptr;
        double *wgl = a.weights ? a.weights + st * a.n : nullptr;
        const bool fresh = a.first && t == 0;
        int flag = (nt >= 1 && nt <= a.n && mt >= 0 && mt <= a.m) ? 0 : 4;
        int iters = 0, evals = 0;
        bool had_root = false, capped = false;

        if (flag == 0) {
            // ---- residuals (main.py:293-296): the target does not enter (:84-85)
            if (method == 1 || method == 2) {
                if (fresh) {
                    for (int q = tid; q < nt; q += SL_THREADS) lsh[q] = 0.6931471805599453;     // -log(0.5)
                } else {
                    const double c0 = k0 ? csh[o0] : 0.0, c1 = k1 ? csh[o1] : 0.0, b = csh[d];
                    for (int r = wave; r < nt; r += SL_NW) {
                        const double *row = X + (size_t)r * d;
                        double x0 = row[o0], x1 = row[o1];
                        x0 = k0 ? x0 : 0.0;
                        x1 = k1 ? x1 : 0.0;
                        const double p = on_dot(x0, x1, c0, c1) + b;
                        if (lane == 0) lsh[r] = p >= 0.0 ? log1p(exp(-p)) : -p + log1p(exp(p));
                    }
                }
                __syncthreads();
            }
            // ---- the weights of this thread's samples tid + 256 j
            double l[E], w[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                const bool v = q < nt;
                l[j] = (method == 1 || method == 2) ? lsh[v ? q : 0] : 0.0;
                w[j] = method == 3 ? wgl[v ? q : 0] : 1.0;
            }
            if (method == 1) {
                iters = on_estep_rlvi<E>(l, w, nt, a.tol, a.maxiter, slots, parity);
            } else if (method == 2) {
                int rc = 1;
                if (eps > 0.0 && eps < 1.0 && (1.0 - eps) * (double)nt > 1.0)
                    rc = mo_estep_rrm<E, ON_STRIDE>(l, w, nt, eps, slots, parity, evals, had_root);
                iters = evals;
                flag = rc == 1 ? 2 : 0;
                capped = rc == 2;
            }
            // the order's indexes: in range, or nothing is read through them
            double bad = 0.0, none = 0.0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int q = tid + j * SL_THREADS;
                if (q < nt) {
                    const int i = ord ? ord[q] : q;
                    const bool ok = (unsigned)i < (unsigned)nt;
                    bad += ok ? 0.0 : 1.0;
                    cidx[q] = ok ? i : 0;
                    lsh[q] = w[j];                                  // (this thread's own entries: read above)
                    if (flag == 0 && method != 3 && wgl) wgl[q] = w[j];
                }
            }
            sl_block_sum2<ON_STRIDE>(bad, none, slots, parity);    // (its barrier: lsh and cidx are whole)
            if (flag == 0 && bad != 0.0) flag = 4;
        }
        if (flag == 0) {
            for (int q = tid; q < nt; q += SL_THREADS) {
                const int i = cidx[q];
                cy[q] = y[i] == 1.0 ? 1.0 : 0.0;
                csw[q] = lsh[i];
            }
        }
        if (tid < 6) cnt[tid] = 0;
        __syncthreads();

        // ---- the pass (one wave): scikit-learn's _plain_sgd, log loss, L2, 'optimal', one epoch in the given order
        if (flag == 0 && wave == 0) {
            double w0 = k0 ? csh[o0] : 0.0, w1 = k1 ? csh[o1] : 0.0;
            double b = csh[d], tt = csh[d + 1], wscale = 1.0;
            const double alpha = a.alpha, oinit = a.oinit;
            int nz = 0;
            double xa[ON_CH], xb[ON_CH], ya[ON_CH], sa[ON_CH], xc[ON_CH], xd[ON_CH], yc[ON_CH], sc[ON_CH];
            auto fetch = [&](int kb, double (&x0)[ON_CH], double (&x1)[ON_CH], double (&yv)[ON_CH],
                             double (&sv)[ON_CH]) {
#pragma unroll
                for (int u = 0; u < ON_CH; ++u) {
                    int k = kb + u;
                    k = k < nt ? k : nt - 1;                        // (past the end: the last sample again, not used)
                    const double *row = X + (size_t)cidx[k] * d;
                    x0[u] = row[o0];
                    x1[u] = row[o1];
                    yv[u] = cy[k];
                    sv[u] = csw[k];
                }
            };
            auto run = [&](int kb, const double (&x0)[ON_CH], const double (&x1)[ON_CH], const double (&yv)[ON_CH],
                           const double (&sv)[ON_CH]) {
#pragma unroll
                for (int u = 0; u < ON_CH; ++u) {
                    if (kb + u < nt) {
                        const double x0v = k0 ? x0[u] : 0.0, x1v = k1 ? x1[u] : 0.0;
                        const double p = wscale * on_dot(x0v, x1v, w0, w1) + b;
                        const double eta = 1.0 / (alpha * (oinit + tt - 1.0));
                        // the log loss's gradient as scikit-learn 1.7.2 computes it (labels 0 / 1, one tail)
                        const double yi = yv[u];
                        const bool body = p > -37.0;
                        const double e = exp(body ? -p : p);
                        double g = body ? ((1.0 - yi) - yi * e) / (1.0 + e) : e - yi;
                        g = g < -ON_MAX_DLOSS ? -ON_MAX_DLOSS : (g > ON_MAX_DLOSS ? ON_MAX_DLOSS : g);
                        const double upd = (-eta * g) * sv[u];
                        const double f = 1.0 - eta * alpha;
                        wscale *= f > 0.0 ? f : 0.0;
                        if (wscale < 1e-9) {
                            w0 *= wscale;
                            w1 *= wscale;
                            wscale = 1.0;
                        }
                        if (upd != 0.0) {
                            const double c = upd / wscale;
                            w0 += x0v * c;
                            w1 += x1v * c;
                            b += upd;
                            ++nz;
                        }
                        tt += 1.0;
                    }
                }
            };
            fetch(0, xa, xb, ya, sa);
            for (int kb = 0; kb < nt; kb += 2 * ON_CH) {
                fetch(kb + ON_CH, xc, xd, yc, sc);
                run(kb, xa, xb, ya, sa);
                fetch(kb + 2 * ON_CH, xa, xb, ya, sa);
                run(kb + ON_CH, xc, xd, yc, sc);
            }
            w0 *= wscale;                                           // coef = w wscale
            w1 *= wscale;
            const double inf = __builtin_inf();
            double nf = (fabs(w0) < inf && fabs(w1) < inf && fabs(b) < inf) ? 0.0 : 1.0;
            nf = wave_max(nf);
            if (k0) csh[o0] = w0;
            if (k1) csh[o1] = w1;
            if (lane == 0) {
                csh[d] = b;
                csh[d + 1] = tt;
                cnt[4] = nf != 0.0 ? 1 : 0;
                cnt[5] = nz;
            }
        }
        __syncthreads();

        // ---- the test rows with the new state (main.py:318-331): prediction = decision value > 0
        if (flag != 4) {
            const double c0 = k0 ? csh[o0] : 0.0, c1 = k1 ? csh[o1] : 0.0, b = csh[d];
            const double *Xt = a.Xt + (size_t)t * a.m * d, *yt = a.yt + (size_t)t * a.m;
            int tp = 0, tn = 0, fp = 0, fn = 0;
            for (int r = wave; r < mt; r += SL_NW) {
                const double *row = Xt + (size_t)r * d;
                double x0 = row[o0], x1 = row[o1];
                x0 = k0 ? x0 : 0.0;
                x1 = k1 ? x1 : 0.0;
                const bool pred = on_dot(x0, x1, c0, c1) + b > 0.0;
                const double yv = yt[r];
                tp += (pred && yv == 1.0) ? 1 : 0;
                tn += (!pred && yv == 0.0) ? 1 : 0;
                fp += (pred && yv == 0.0) ? 1 : 0;
                fn += (!pred && yv == 1.0) ? 1 : 0;
            }
            if (lane == 0 && mt > 0) {
                atomicAdd(&cnt[0], tp);
                atomicAdd(&cnt[1], tn);
                atomicAdd(&cnt[2], fp);
                atomicAdd(&cnt[3], fn);
            }
        }
        __syncthreads();
        if (tid < 4) a.counts[st * 4 + tid] = cnt[tid];
        if (tid < d + 2) a.state_out[st * (size_t)(d + 2) + tid] = csh[tid];
        if (tid == 0) {
            int fl = flag;
            if (fl == 0 && capped) fl = 3;
            if ((fl == 0 || fl == 3) && cnt[4]) fl = 1;
            a.info[st * 4 + 0] = iters;
            a.info[st * 4 + 1] = had_root ? 1 : 0;
            a.info[st * 4 + 2] = cnt[5];
            a.info[st * 4 + 3] = fl;
        }
        __syncthreads();                                            // (cnt is zeroed again by the next batch)
    }
}

static size_t on_lds_bytes(int npad) {
    return (size_t)(ON_STATE + sl_slot_doubles(ON_STRIDE) + 3 * npad) * sizeof(double) + (size_t)(npad + 8) * sizeof(int);
}

// 1 / (eta0 alpha) of scikit-learn's 'optimal' schedule: typw = sqrt(1 / sqrt(alpha)), eta0 = typw / max(1, dloss(1,
// -typw))
static double on_optimal_init(double alpha) {
    const double typw = sqrt(1.0 / sqrt(alpha));
    const double e = exp(typw);
    const double dl = -e / (1.0 + e);
    const double eta0 = typw / (dl > 1.0 ? dl : 1.0);
    return 1.0 / (eta0 * alpha);
}

static int on_launch(OnArgs &a, int S, void *stream) {
    a.npad = sl_pad64(a.n);
    a.oinit = on_optimal_init(a.alpha);
    return sl_samples_per_thread(a.n, [&](auto f) {
        return sl_launch(online_sgd_kernel<decltype(f)::E>, S, on_lds_bytes(a.npad), static_cast<hipStream_t>(stream), a);
    });
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_online_step_f64(const double *X, const double *y, const int32_t *order, int64_t n, int64_t d,
                                    int method, double eps, int first, double *state, const double *Xt,
                                    const double *yt, int64_t m, double alpha, double tol, int maxiter,
                                    double *sample_weight, int32_t *counts, int32_t *info, void *stream) {
    const bool params_ok = m >= 0 && maxiter >= 0 && method >= 0 && method <= 3 && alpha > 0.0 &&
                           (method != 2 || (eps > 0.0 && eps < 1.0));
    if (const int e = sl_check_args({X, y, state, counts, info, sl_when(m > 0, Xt), sl_when(m > 0, yt),
                                     sl_when(method == 3, sample_weight)},
                                    1, n, d, params_ok, n <= SL_MAXN && m <= SL_MAXN && d <= ON_MAXD,
                                    {X, y, state, Xt, yt, sample_weight}, {order, counts, info}))
        return e;
    OnArgs a = {};
    a.X = X; a.y = y; a.Xt = Xt; a.yt = yt;
    a.rows = nullptr; a.orders = order;
    a.state_in = state; a.state_out = state;
    a.weights = sample_weight; a.counts = counts; a.info = info;
    a.T = 1; a.n = (int)n; a.m = (int)m; a.d = (int)d; a.first = first ? 1 : 0; a.maxiter = maxiter;
    a.alpha = alpha; a.tol = tol;
    a.method[0] = method; a.eps[0] = eps;
    return on_launch(a, 1, stream);
}

extern "C" int rlvi_online_stream_f64(const double *X, const double *y, const double *Xt, const double *yt,
                                      const int32_t *rows, const int32_t *orders, int64_t T, int64_t n, int64_t m,
                                      int64_t d, const int32_t *methods, const double *eps, int64_t S, double alpha,
                                      double tol, int maxiter, double *state_hist, int32_t *counts, double *weights,
                                      int32_t *info, void *stream) {
    if (const int e = sl_check_values({X, y, methods, state_hist, counts, info, sl_when(m > 0, Xt), sl_when(m > 0, yt)},
                                      1, n, d, T > 0 && S > 0 && m >= 0 && maxiter >= 0 && alpha > 0.0,
                                      S <= ON_MAXS && T <= ON_MAXT && n <= SL_MAXN && m <= SL_MAXN && d <= ON_MAXD))
        return e;
    // the classifiers' own checks: behind the limits (S), in front of the alignment
    OnArgs a = {};
    for (int64_t s = 0; s < S; ++s) {
        const int me = methods[s];
        if (me < 0 || me > 3) return RLVI_E_SHAPE;
        if (me == 3 && !weights) return RLVI_E_NULL;
        if (me == 2 && (!eps || !(eps[s] > 0.0 && eps[s] < 1.0))) return eps ? RLVI_E_SHAPE : RLVI_E_NULL;
        a.method[s] = me;
        a.eps[s] = eps ? eps[s] : 0.0;
    }
    if (sl_misaligned({X, y, Xt, yt, state_hist, weights}, {rows, orders, counts, info})) return RLVI_E_ALIGN;
    a.X = X; a.y = y; a.Xt = Xt; a.yt = yt;
    a.rows = rows; a.orders = orders;
    a.state_in = nullptr; a.state_out = state_hist;
    a.weights = weights; a.counts = counts; a.info = info;
    a.T = (int)T; a.n = (int)n; a.m = (int)m; a.d = (int)d; a.first = 1; a.maxiter = maxiter;
    a.alpha = alpha; a.tol = tol;
    return on_launch(a, (int)S, stream);
}
