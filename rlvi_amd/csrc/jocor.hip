// JoCoR's joint loss over two logit blocks, forward and backward (deep-learning/methods/train_jocor.py:17-43).
//
// For every row i of the two blocks z1 (model 1) and z2 (model 2), with p = softmax(z1_i), q = softmax(z2_i),
// lp / lq their log-softmax, lambda = co_lambda and y_i the label, the reference forms
//     loss_pick_i = (1-lambda) CE1_i + (1-lambda) CE2_i + lambda K_qp + lambda K_pq          (:30-34)
// where K_qp = mean_b KL(q_b || p_b) and K_pq = mean_b KL(p_b || q_b) are BATCH MEANS, one scalar each:
// kl_loss_compute(..., reduce='none') tests `if reduce:` and the string 'none' is truthy (:23), so both calls
// return torch.mean(torch.sum(kl, 1)), not a vector per row.  The k = int((1 - forget_rate) B) smallest loss_pick
// are kept (:36-40) and L = their mean (:42).  Reproduced as the reference runs it (not as the JoCoR paper writes
// it, with the KL per row): the KL scalars shift every row alike, so the selection is by the cross-entropies,
// and every row -- selected or not -- gets the KL gradient, lambda / B (p - q + p (lp - lq - KL(p||q)_i)) for z1.
//
// Three launches, no host round trip:
//   pass 1 (jocor_rows_kernel): reads both blocks once; per row max, log-sum-exp, CE1, CE2, KL(p||q)_i and
//     KL(q||p)_i (a second sweep over the row in registers) and model 1's top-1; writes
//     a_i = (1-lambda) CE1_i + (1-lambda) CE2_i to loss_pick[i] and one fp64 record {sum KL(q||p), sum KL(p||q),
//     hits} per workgroup (no atomics: fixed-order sums);
//   selection (jocor_select_kernel, one workgroup): reduces the records in a fixed order, forms every loss_pick_i
//     with the reference's fp32 rounding order ((a_i + lambda K_qp) + lambda K_pq), takes the k smallest by the
//     radix select of rlvi_select.h (equal values in index order), writes the 0/1 selection, loss_pick and
//     out = {L, K_qp, K_pq, top-1 % of model 1};
//   pass 2 (jocor_grad_kernel): re-reads both blocks and writes both gradients in the logits' dtype (one rounding,
//     nearest even), scaled by the upstream gradient and an optional loss scale read on the device once per wave.
// A row of at most 16 G elements lives in the registers of a group of G lanes (V-element vectors); longer rows
// take a wave per row that sweeps the row from memory (the second and later sweeps are cache hits).
#include "rlvi_select.h"

namespace rlvi {

constexpr int JC_THREADS = 256;
constexpr int JC_WAVES = JC_THREADS / WAVE;
constexpr int JC_ELEMS = 16;                 // elements per lane and block of the register form (JC_ELEMS / V vectors)

// One row in the registers of G lanes: lane g holds the vectors k*G + g, k < kact <= JC_KMAX.  After
// stats(), d1 / d2 hold z - max (dead slots -inf) and the row's log-sum-exp parts and KL terms are set.
template <typename T, int V, int G>
struct RegRow {
    static constexpr int JC_KMAX = JC_ELEMS / V;
    float d1[JC_KMAX][V], d2[JC_KMAX][V];
    bool live[JC_KMAX];
    float ls1, ls2;              // log sum exp(z - max)
    float s1, s2;                // sum exp(z - max)
    float kl_pq, kl_qp;          // KL(p||q)_i, KL(q||p)_i
    int earlier;                 // columns before y that attain model 1's maximum

    __device__ __forceinline__ void load(const T *z1, const T *z2, int C, int kact, int g) {
#pragma unroll
        for (int k = 0; k < JC_KMAX; ++k) {
            const int col = (k * G + g) * V;
            live[k] = k < kact && col < C;
            const int c = live[k] ? col : g * V < C ? g * V : 0;     // dead slots re-read a live vector
            VecIO<T, V>::load(z1 + c, d1[k]);
            VecIO<T, V>::load(z2 + c, d2[k]);
        }
    }

    __device__ __forceinline__ void stats(int g, int y) {
        const float NEG_INF = -__builtin_inff();
        float m1 = NEG_INF, m2 = NEG_INF;
#pragma unroll
        for (int k = 0; k < JC_KMAX; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                d1[k][j] = live[k] ? d1[k][j] : NEG_INF;
                d2[k][j] = live[k] ? d2[k][j] : NEG_INF;
                m1 = fmaxf(m1, d1[k][j]);
                m2 = fmaxf(m2, d2[k][j]);
            }
        m1 = group_max<G>(m1);
        m2 = group_max<G>(m2);
        float a1 = 0.0f, a2 = 0.0f;
#pragma unroll
        for (int k = 0; k < JC_KMAX; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                d1[k][j] -= m1;
                d2[k][j] -= m2;
                a1 += mexp(d1[k][j]);
                a2 += mexp(d2[k][j]);
            }
        s1 = group_sum<G>(a1);
        s2 = group_sum<G>(a2);
        ls1 = logf(s1);
        ls2 = logf(s2);
        const float r1 = 1.0f / s1, r2 = 1.0f / s2;
        float kpq = 0.0f, kqp = 0.0f;
        int ea = 0;
#pragma unroll
        for (int k = 0; k < JC_KMAX; ++k) {
            const int col = (k * G + g) * V;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (live[k]) {
                    // in log space: a softmax entry that underflowed to 0 contributes 0 (torch's xlogy)
                    const float diff = (d1[k][j] - ls1) - (d2[k][j] - ls2);       // lp - lq
                    kpq += (mexp(d1[k][j]) * r1) * diff;
                    kqp -= (mexp(d2[k][j]) * r2) * diff;
                    ea += (d1[k][j] == 0.0f && col + j < y) ? 1 : 0;
                }
            }
        }
        kl_pq = group_sum<G>(kpq);
        kl_qp = group_sum<G>(kqp);
        earlier = group_allreduce<G>(ea, FAdd());
        m1_ = m1;
        m2_ = m2;
    }
    float m1_, m2_;
};

// Per-row scalars of pass 1 from the row statistics: a_i = (1-lambda) CE1 + (1-lambda) CE2 in the reference's
// rounding order (each product rounded, then the sum; no fused multiply-add)
__device__ __forceinline__ float jc_pick_ce(float ce1, float ce2, float c1) {
    return __fadd_rn(__fmul_rn(ce1, c1), __fmul_rn(ce2, c1));
}

// Block record {sum KL(q||p)_i, sum KL(p||q)_i, hits, 0}: fixed-order sums, one record per workgroup
__device__ __forceinline__ void jc_write_record(double *part, double kqp, double kpq, double hits) {
    __shared__ double sh[3 * JC_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    kqp = wave_sum(kqp);
    kpq = wave_sum(kpq);
    hits = wave_sum(hits);
    if (lane == 0) { sh[3 * wave] = kqp; sh[3 * wave + 1] = kpq; sh[3 * wave + 2] = hits; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int w = 0; w < JC_WAVES; ++w) { t0 += sh[3 * w]; t1 += sh[3 * w + 1]; t2 += sh[3 * w + 2]; }
        double *p = part + (size_t)PART_STRIDE * blockIdx.x;
        p[0] = t0; p[1] = t1; p[2] = t2; p[3] = 0.0;
    }
}

// ---- pass 1, register rows --------------------------------------------------------------------------------
template <typename T, int V, int G>
__global__ __launch_bounds__(JC_THREADS) void jocor_rows_kernel(
    const T *__restrict__ z1, int64_t ld1, const T *__restrict__ z2, int64_t ld2, const int64_t *__restrict__ labels,
    int64_t B, int C, int kact, float c1, float *__restrict__ loss_pick, double *__restrict__ part,
    int32_t *__restrict__ status) {
    constexpr int R = WAVE / G;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int g = lane & (G - 1), sub = lane / G;
    double kqp = 0.0, kpq = 0.0, hits = 0.0;
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * JC_WAVES * R;
    for (int64_t row0 = ((int64_t)blockIdx.x * JC_WAVES + wave) * R; row0 < B; row0 += stride) {
        const int64_t row = row0 + sub;
        const bool valid = row < B;
        const int64_t rr = valid ? row : B - 1;     // padding rows recompute the last row, store nothing
        int64_t y64 = labels[rr];
        RegRow<T, V, G> r;
        r.load(z1 + rr * ld1, z2 + rr * ld2, C, kact, g);
        const bool y_ok = y64 >= 0 && y64 < C;
        bad = bad || (valid && !y_ok);
        const int y = y_ok ? (int)y64 : 0;
        const float zy1 = load1(z1 + rr * ld1, y), zy2 = load1(z2 + rr * ld2, y);
        r.stats(g, y);
        if (g == 0 && valid) {
            // CE = log sum exp(z - max) - (z_y - max), as torch evaluates it; a label out of range gives NaN
            const float nan = __builtin_nanf("");
            const float ce1 = y_ok ? r.ls1 - (zy1 - r.m1_) : nan;
            const float ce2 = y_ok ? r.ls2 - (zy2 - r.m2_) : nan;
            loss_pick[row] = jc_pick_ce(ce1, ce2, c1);
            kqp += (double)r.kl_qp;
            kpq += (double)r.kl_pq;
            hits += (y_ok && zy1 == r.m1_ && r.earlier == 0) ? 1.0 : 0.0;
        }
    }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    jc_write_record(part, kqp, kpq, hits);
}

// ---- pass 2, register rows --------------------------------------------------------------------------------
template <typename T, int V, int G>
__global__ __launch_bounds__(JC_THREADS) void jocor_grad_kernel(
    const T *__restrict__ z1, int64_t ld1, const T *__restrict__ z2, int64_t ld2, const int64_t *__restrict__ labels,
    const float *__restrict__ sel, int64_t B, int C, int kact, int64_t k, float c1, float lam,
    const float *__restrict__ grad_out, const float *__restrict__ grad_scale, T *__restrict__ g1, int64_t ldg1,
    T *__restrict__ g2, int64_t ldg2) {
    constexpr int R = WAVE / G;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int g = lane & (G - 1), sub = lane / G;
    const float gain = grad_gain(grad_out != nullptr ? *grad_out : 1.0f, grad_scale);
    // d L / d loss_pick_i = g / k on the selected rows; the KL scalars collect it from all k of them: g lambda / B.
    // k = 0: torch.mean of nothing is NaN and nothing flows back -- both gradients are zero.
    const float c_ce = k > 0 ? (gain / (float)k) * c1 : 0.0f;
    const float c_kl = k > 0 ? gain * lam / (float)B : 0.0f;
    const int64_t stride = (int64_t)gridDim.x * JC_WAVES * R;
    for (int64_t row0 = ((int64_t)blockIdx.x * JC_WAVES + wave) * R; row0 < B; row0 += stride) {
        const int64_t row = row0 + sub;
        const bool valid = row < B;
        const int64_t rr = valid ? row : B - 1;
        const int64_t y64 = labels[rr];
        const float s = sel[rr];
        RegRow<T, V, G> r;
        r.load(z1 + rr * ld1, z2 + rr * ld2, C, kact, g);
        const bool y_ok = y64 >= 0 && y64 < C;
        const int y = y_ok ? (int)y64 : -1;             // no one-hot column for a label out of range
        r.stats(g, y);
        if (!valid) continue;
        const float cs = (s != 0.0f && y_ok) ? c_ce : 0.0f;
        const float r1 = 1.0f / r.s1, r2 = 1.0f / r.s2;
#pragma unroll
        for (int kk = 0; kk < RegRow<T, V, G>::JC_KMAX; ++kk) {
            if (!r.live[kk]) continue;
            const int col = (kk * G + g) * V;
            float o1[V], o2[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float p = mexp(r.d1[kk][j]) * r1, q = mexp(r.d2[kk][j]) * r2;
                const float diff = (r.d1[kk][j] - r.ls1) - (r.d2[kk][j] - r.ls2);     // lp - lq
                const float hot = col + j == y ? 1.0f : 0.0f;
                o1[j] = cs * (p - hot) + c_kl * ((p - q) + p * (diff - r.kl_pq));
                o2[j] = cs * (q - hot) + c_kl * ((q - p) + q * (-diff - r.kl_qp));
            }
            if (g1 != nullptr) VecIO<T, V>::store(g1 + rr * ldg1 + col, o1);
            if (g2 != nullptr) VecIO<T, V>::store(g2 + rr * ldg2 + col, o2);
        }
    }
}

// ---- long rows: a wave per row, every sweep from memory ---------------------------------------------------
struct LongStats {
    float m1, m2, ls1, ls2, s1, s2, kl_pq, kl_qp;
    int earlier;
};

template <typename T>
__device__ __forceinline__ LongStats long_stats(const T *z1, const T *z2, int C, int lane, int y) {
    LongStats st;
    float m1 = -__builtin_inff(), m2 = -__builtin_inff();
    for (int c = lane; c < C; c += WAVE) { m1 = fmaxf(m1, load1(z1, c)); m2 = fmaxf(m2, load1(z2, c)); }
    m1 = wave_max(m1);
    m2 = wave_max(m2);
    float a1 = 0.0f, a2 = 0.0f;
    for (int c = lane; c < C; c += WAVE) { a1 += mexp(load1(z1, c) - m1); a2 += mexp(load1(z2, c) - m2); }
    st.s1 = wave_sum(a1);
    st.s2 = wave_sum(a2);
    st.ls1 = logf(st.s1);
    st.ls2 = logf(st.s2);
    const float r1 = 1.0f / st.s1, r2 = 1.0f / st.s2;
    float kpq = 0.0f, kqp = 0.0f;
    int ea = 0;
    for (int c = lane; c < C; c += WAVE) {
        const float e1 = load1(z1, c) - m1, e2 = load1(z2, c) - m2;
        const float diff = (e1 - st.ls1) - (e2 - st.ls2);
        kpq += (mexp(e1) * r1) * diff;
        kqp -= (mexp(e2) * r2) * diff;
        ea += (e1 == 0.0f && c < y) ? 1 : 0;
    }
    st.kl_pq = wave_sum(kpq);
    st.kl_qp = wave_sum(kqp);
    st.earlier = wave_sum(ea);
    st.m1 = m1;
    st.m2 = m2;
    return st;
}

template <typename T>
__global__ __launch_bounds__(JC_THREADS) void jocor_rows_long_kernel(
    const T *__restrict__ z1, int64_t ld1, const T *__restrict__ z2, int64_t ld2, const int64_t *__restrict__ labels,
    int64_t B, int C, float c1, float *__restrict__ loss_pick, double *__restrict__ part,
    int32_t *__restrict__ status) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    double kqp = 0.0, kpq = 0.0, hits = 0.0;
    bool bad = false;
    for (int64_t row = (int64_t)blockIdx.x * JC_WAVES + wave; row < B; row += (int64_t)gridDim.x * JC_WAVES) {
        const int64_t y64 = labels[row];
        const bool y_ok = y64 >= 0 && y64 < C;
        bad = bad || !y_ok;
        const int y = y_ok ? (int)y64 : 0;
        const T *r1 = z1 + row * ld1, *r2 = z2 + row * ld2;
        const LongStats st = long_stats(r1, r2, C, lane, y);
        if (lane == 0) {
            const float zy1 = load1(r1, y), zy2 = load1(r2, y);
            const float nan = __builtin_nanf("");
            const float ce1 = y_ok ? st.ls1 - (zy1 - st.m1) : nan;
            const float ce2 = y_ok ? st.ls2 - (zy2 - st.m2) : nan;
            loss_pick[row] = jc_pick_ce(ce1, ce2, c1);
            kqp += (double)st.kl_qp;
            kpq += (double)st.kl_pq;
            hits += (y_ok && zy1 == st.m1 && st.earlier == 0) ? 1.0 : 0.0;
        }
    }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    jc_write_record(part, kqp, kpq, hits);
}

template <typename T>
__global__ __launch_bounds__(JC_THREADS) void jocor_grad_long_kernel(
    const T *__restrict__ z1, int64_t ld1, const T *__restrict__ z2, int64_t ld2, const int64_t *__restrict__ labels,
    const float *__restrict__ sel, int64_t B, int C, int64_t k, float c1, float lam,
    const float *__restrict__ grad_out, const float *__restrict__ grad_scale, T *__restrict__ g1, int64_t ldg1,
    T *__restrict__ g2, int64_t ldg2) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const float gain = grad_gain(grad_out != nullptr ? *grad_out : 1.0f, grad_scale);
    const float c_ce = k > 0 ? (gain / (float)k) * c1 : 0.0f;
    const float c_kl = k > 0 ? gain * lam / (float)B : 0.0f;
    for (int64_t row = (int64_t)blockIdx.x * JC_WAVES + wave; row < B; row += (int64_t)gridDim.x * JC_WAVES) {
        const int64_t y64 = labels[row];
        const bool y_ok = y64 >= 0 && y64 < C;
        const int y = y_ok ? (int)y64 : -1;
        const T *r1 = z1 + row * ld1, *r2 = z2 + row * ld2;
        const LongStats st = long_stats(r1, r2, C, lane, y);
        const float cs = (sel[row] != 0.0f && y_ok) ? c_ce : 0.0f;
        const float i1 = 1.0f / st.s1, i2 = 1.0f / st.s2;
        for (int c = lane; c < C; c += WAVE) {
            const float e1 = load1(r1, c) - st.m1, e2 = load1(r2, c) - st.m2;
            const float p = mexp(e1) * i1, q = mexp(e2) * i2;
            const float diff = (e1 - st.ls1) - (e2 - st.ls2);
            const float hot = c == y ? 1.0f : 0.0f;
            float o[1];
            if (g1 != nullptr) {
                o[0] = cs * (p - hot) + c_kl * ((p - q) + p * (diff - st.kl_pq));
                VecIO<T, 1>::store(g1 + row * ldg1 + c, o);
            }
            if (g2 != nullptr) {
                o[0] = cs * (q - hot) + c_kl * ((q - p) + q * (-diff - st.kl_qp));
                VecIO<T, 1>::store(g2 + row * ldg2 + c, o);
            }
        }
    }
}

// ---- selection: one workgroup -----------------------------------------------------------------------------
// The records of pass 1 in a fixed order -> K_qp, K_pq (rounded to fp32, as the reference's 0-dim tensors are);
// loss_pick_i = (a_i + lambda K_qp) + lambda K_pq in fp32; the k smallest by select_smallest_block (rlvi_select.h:
// equal values in index order, NaN last); L = their mean (fp64 sum in a fixed order).  Reads a_i from loss_pick and
// writes loss_pick_i back over it.  Clears the records it consumed.
__global__ __launch_bounds__(SEL_BLOCK) void jocor_select_kernel(float *__restrict__ loss_pick, int64_t n,
                                                                 int64_t k, float lam, double *__restrict__ part,
                                                                 int nrec, float *__restrict__ sel,
                                                                 float *__restrict__ out) {
    __shared__ double shd[3 * SEL_NW];
    __shared__ float sh_k[2];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;

    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    for (int i = tid; i < nrec; i += SEL_BLOCK) {
        r0 += part[(size_t)PART_STRIDE * i];
        r1 += part[(size_t)PART_STRIDE * i + 1];
        r2 += part[(size_t)PART_STRIDE * i + 2];
    }
    r0 = wave_sum(r0);
    r1 = wave_sum(r1);
    r2 = wave_sum(r2);
    if (lane == 0) { shd[3 * wave] = r0; shd[3 * wave + 1] = r1; shd[3 * wave + 2] = r2; }
    __syncthreads();
    for (int i = tid; i < nrec; i += SEL_BLOCK)
#pragma unroll
        for (int c = 0; c < PART_STRIDE; ++c) part[(size_t)PART_STRIDE * i + c] = 0.0;
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < SEL_NW; ++w) { t0 += shd[3 * w]; t1 += shd[3 * w + 1]; t2 += shd[3 * w + 2]; }
        const float kqp = (float)(t0 / (double)n), kpq = (float)(t1 / (double)n);
        sh_k[0] = __fmul_rn(lam, kqp);
        sh_k[1] = __fmul_rn(lam, kpq);
        out[1] = kqp;
        out[2] = kpq;
        out[3] = (float)(t2 * 100.0 / (double)n);
    }
    __syncthreads();
    const float lk1 = sh_k[0], lk2 = sh_k[1];

    double acc = 0.0;                            // the kept values of this thread's rows
    select_smallest_block(
        loss_pick, n, k, [&](float a) { return __fadd_rn(__fadd_rn(a, lk1), lk2); },
        [&](int64_t i, float v, bool keep) {
            loss_pick[i] = v;
            sel[i] = keep ? 1.0f : 0.0f;
            if (keep) acc += (double)v;
        });
    acc = wave_sum(acc);
    __syncthreads();
    if (lane == 0) shd[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < SEL_NW; ++w) t += shd[w];
        out[0] = k <= 0 ? __builtin_nanf("") : (float)(t / (double)(k >= n ? n : k));
    }
}

// ---- launchers --------------------------------------------------------------------------------------------
struct JcShape {
    int V, G, kact;   // G == 0: long rows
};

template <typename T>
static JcShape jc_pick_shape(const void *z1, int64_t ld1, const void *z2, int64_t ld2, const void *g1, int64_t ldg1,
                             const void *g2, int64_t ldg2, int64_t C) {
    constexpr int VMAX = 16 / (int)sizeof(T);
    auto ok = [&](int v) { return vec_fits<T>(v, C, {{z1, ld1}, {z2, ld2}, {g1, ldg1}, {g2, ldg2}}); };
    const int V = ok(VMAX) ? VMAX : ok(2) ? 2 : 1;
    const int64_t nv = C / V;
    for (int G : {4, 16, 64})
        if (nv <= (int64_t)G * (JC_ELEMS / V)) return {V, G, (int)((nv + G - 1) / G)};
    return {1, 0, 0};
}

static int64_t jc_blocks(int64_t B, int rows_per_block, int64_t cap) {
    int64_t nb = (B + rows_per_block - 1) / rows_per_block;
    return nb < cap ? nb : cap;
}

template <typename T>
static int jc_check(const T *z1, int64_t ld1, const T *z2, int64_t ld2, const int64_t *labels, int64_t B,
                    int64_t C) {
    if (!z1 || !z2 || !labels) return RLVI_E_NULL;
    if (B <= 0 || C <= 0 || ld1 < C || ld2 < C) return RLVI_E_SHAPE;
    if (C > (1 << 20) || B >= ((int64_t)1 << 31)) return RLVI_E_LIMIT;
    if (((uintptr_t)labels & 7) || ((uintptr_t)z1 % sizeof(T)) || ((uintptr_t)z2 % sizeof(T))) return RLVI_E_ALIGN;
    return 0;
}

template <typename T>
static int jocor_fwd(const T *z1, int64_t ld1, const T *z2, int64_t ld2, const int64_t *labels, int64_t B, int64_t C,
                     int64_t k, float co_lambda, float *loss_pick, float *sel, float *out, void *ws, void *stream) {
    int rc = jc_check(z1, ld1, z2, ld2, labels, B, C);
    if (rc) return rc;
    if (!loss_pick || !sel || !out || !ws) return RLVI_E_NULL;
    if (k < 0) return RLVI_E_SHAPE;
    if (((uintptr_t)loss_pick & 3) || ((uintptr_t)sel & 3) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 255))
        return RLVI_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    double *part = reinterpret_cast<double *>(base + WS_PART2_OFF);
    int32_t *status = reinterpret_cast<int32_t *>(base);
    // the reference's (1 - co_lambda) and co_lambda: Python floats that multiply fp32 tensors, i.e. fp32 factors
    const float c1 = (float)(1.0 - (double)co_lambda), lam = co_lambda;
    const JcShape sh = jc_pick_shape<T>(z1, ld1, z2, ld2, nullptr, 0, nullptr, 0, C);
    const int Ci = (int)C;
    int64_t nb;
    if (sh.G == 0) {
        nb = jc_blocks(B, JC_WAVES, MSTEP_MAX_BLOCKS);
        rc = launch(jocor_rows_long_kernel<T>, dim3((unsigned)nb), dim3(JC_THREADS), 0, st, z1, ld1, z2, ld2, labels,
                    B, Ci, c1, loss_pick, part, status);
    } else {
        nb = jc_blocks(B, JC_WAVES * (WAVE / sh.G), MSTEP_MAX_BLOCKS);
#define RLVI_JR(V_, G_)                                                                                        \
    rc = launch(jocor_rows_kernel<T, V_, G_>, dim3((unsigned)nb), dim3(JC_THREADS), 0, st, z1, ld1, z2, ld2, labels, \
                B, Ci, sh.kact, c1, loss_pick, part, status)
#define RLVI_JR_G(V_)                          \
    if (sh.G == 4) RLVI_JR(V_, 4);             \
    else if (sh.G == 16) RLVI_JR(V_, 16);      \
    else RLVI_JR(V_, 64)
        constexpr int VMAX = 16 / (int)sizeof(T);
        if (sh.V == VMAX) { RLVI_JR_G(VMAX); }
        else if (sh.V == 2) { RLVI_JR_G(2); }
        else { RLVI_JR_G(1); }
#undef RLVI_JR_G
#undef RLVI_JR
    }
    if (rc) return rc;
    return launch(jocor_select_kernel, dim3(1), dim3(SEL_BLOCK), 0, st, loss_pick, B, k, lam, part, (int)nb, sel,
                  out);
}

template <typename T>
static int jocor_bwd(const T *z1, int64_t ld1, const T *z2, int64_t ld2, const int64_t *labels, const float *sel,
                     int64_t B, int64_t C, int64_t k, float co_lambda, const float *grad_out, const float *grad_scale,
                     T *g1, int64_t ldg1, T *g2, int64_t ldg2, void *stream) {
    int rc = jc_check(z1, ld1, z2, ld2, labels, B, C);
    if (rc) return rc;
    if (!sel) return RLVI_E_NULL;
    if (k < 0 || (g1 && ldg1 < C) || (g2 && ldg2 < C)) return RLVI_E_SHAPE;
    if (((uintptr_t)sel & 3) || ((uintptr_t)grad_out & 3) || ((uintptr_t)grad_scale & 3) ||
        ((uintptr_t)g1 % sizeof(T)) || ((uintptr_t)g2 % sizeof(T)))
        return RLVI_E_ALIGN;
    if (!g1 && !g2) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float c1 = (float)(1.0 - (double)co_lambda), lam = co_lambda;
    const JcShape sh = jc_pick_shape<T>(z1, ld1, z2, ld2, g1, ldg1, g2, ldg2, C);
    const int Ci = (int)C;
    const int64_t cap = 8ll * device_info().cus;
    if (sh.G == 0) {
        const int64_t nb = jc_blocks(B, JC_WAVES, cap);
        return launch(jocor_grad_long_kernel<T>, dim3((unsigned)nb), dim3(JC_THREADS), 0, st, z1, ld1, z2, ld2, labels,
                      sel, B, Ci, k, c1, lam, grad_out, grad_scale, g1, ldg1, g2, ldg2);
    }
    const int64_t nb = jc_blocks(B, JC_WAVES * (WAVE / sh.G), cap);
#define RLVI_JG(V_, G_)                                                                                        \
    rc = launch(jocor_grad_kernel<T, V_, G_>, dim3((unsigned)nb), dim3(JC_THREADS), 0, st, z1, ld1, z2, ld2, labels, \
                sel, B, Ci, sh.kact, k, c1, lam, grad_out, grad_scale, g1, ldg1, g2, ldg2)
#define RLVI_JG_G(V_)                          \
    if (sh.G == 4) RLVI_JG(V_, 4);             \
    else if (sh.G == 16) RLVI_JG(V_, 16);      \
    else RLVI_JG(V_, 64)
    constexpr int VMAX = 16 / (int)sizeof(T);
    if (sh.V == VMAX) { RLVI_JG_G(VMAX); }
    else if (sh.V == 2) { RLVI_JG_G(2); }
    else { RLVI_JG_G(1); }
#undef RLVI_JG_G
#undef RLVI_JG
    return rc;
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_jocor_fwd_f32(const float *logits1, int64_t ld1, const float *logits2, int64_t ld2,
                                  const int64_t *labels, int64_t B, int64_t C, int64_t k, float co_lambda,
                                  float *loss_pick, float *sel, float *out, void *ws, void *stream) {
    return jocor_fwd<float>(logits1, ld1, logits2, ld2, labels, B, C, k, co_lambda, loss_pick, sel, out, ws, stream);
}
extern "C" int rlvi_jocor_fwd_bf16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                                   const int64_t *labels, int64_t B, int64_t C, int64_t k, float co_lambda,
                                   float *loss_pick, float *sel, float *out, void *ws, void *stream) {
    return jocor_fwd<uint16_t>(logits1, ld1, logits2, ld2, labels, B, C, k, co_lambda, loss_pick, sel, out, ws,
                               stream);
}
extern "C" int rlvi_jocor_fwd_f16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                                  const int64_t *labels, int64_t B, int64_t C, int64_t k, float co_lambda,
                                  float *loss_pick, float *sel, float *out, void *ws, void *stream) {
    return jocor_fwd<f16_t>(reinterpret_cast<const f16_t *>(logits1), ld1, reinterpret_cast<const f16_t *>(logits2),
                            ld2, labels, B, C, k, co_lambda, loss_pick, sel, out, ws, stream);
}

extern "C" int rlvi_jocor_bwd_f32(const float *logits1, int64_t ld1, const float *logits2, int64_t ld2,
                                  const int64_t *labels, const float *sel, int64_t B, int64_t C, int64_t k,
                                  float co_lambda, const float *grad_out, const float *grad_scale, float *grad1,
                                  int64_t ldg1, float *grad2, int64_t ldg2, void *stream) {
    return jocor_bwd<float>(logits1, ld1, logits2, ld2, labels, sel, B, C, k, co_lambda, grad_out, grad_scale, grad1,
                            ldg1, grad2, ldg2, stream);
}
extern "C" int rlvi_jocor_bwd_bf16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                                   const int64_t *labels, const float *sel, int64_t B, int64_t C, int64_t k,
                                   float co_lambda, const float *grad_out, const float *grad_scale, uint16_t *grad1,
                                   int64_t ldg1, uint16_t *grad2, int64_t ldg2, void *stream) {
    return jocor_bwd<uint16_t>(logits1, ld1, logits2, ld2, labels, sel, B, C, k, co_lambda, grad_out, grad_scale,
                               grad1, ldg1, grad2, ldg2, stream);
}
extern "C" int rlvi_jocor_bwd_f16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                                  const int64_t *labels, const float *sel, int64_t B, int64_t C, int64_t k,
                                  float co_lambda, const float *grad_out, const float *grad_scale, uint16_t *grad1,
                                  int64_t ldg1, uint16_t *grad2, int64_t ldg2, void *stream) {
    return jocor_bwd<f16_t>(reinterpret_cast<const f16_t *>(logits1), ld1, reinterpret_cast<const f16_t *>(logits2),
                            ld2, labels, sel, B, C, k, co_lambda, grad_out, grad_scale,
                            reinterpret_cast<f16_t *>(grad1), ldg1, reinterpret_cast<f16_t *>(grad2), ldg2, stream);
}
