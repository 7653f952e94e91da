// M-step over one mini-batch: per-sample NLL + top-1 + residual scatter + pi gather +
// pi-weighted loss + gradient w.r.t. the logits, in ONE streaming pass over the logit block.
//
// Replaces deep-learning/methods/train_rlvi.py:85,89,90,92,93-94 and the autograd backward
// reached from :96.
//
// Bound: HBM.  Algorithmic bytes per sample = 2*C*s + 24 (logits read + grad write + label 8 +
// index 8 + pi gather 4 + residual scatter 4), s = 4 (fp32) or 2 (bf16, fp16).
//
// Mapping (gfx950, 64-lane waves): a row is owned by a group of G consecutive lanes, every lane
// holding K vectors of V elements (16 B per lane per load when the row pitch allows), so a wave
// works on 64/G rows at once and a row is read exactly once and written exactly once.  Row
// reductions (max, sum-exp, arg-max) are butterfly shuffles inside the lane group.
#include <stdlib.h>

#include <type_traits>

#include "rlvi_common.h"

namespace rlvi {

constexpr int MSTEP_THREADS = 256;
constexpr int MSTEP_WAVES = MSTEP_THREADS / WAVE;

// Per-block partial record.  accum == 0: overwrite (a finalize launch follows); accum == 1: add
// to what earlier mini-batches of this epoch left there (rlvi_epoch_end_f32 reduces and clears).
// Every block owns its record, so there are no atomics and the sums are order-deterministic.
__device__ __forceinline__ void write_partial(double *part, double ta, double th, float inv_scale,
                                              double inv_rows100, int accum) {
    double *p = part + (size_t)PART_STRIDE * blockIdx.x;
    const double v0 = ta * (double)inv_scale, v1 = th * inv_rows100;
    if (accum) {
        // four no-return fp64 adds at the memory side instead of a read-modify-write: the record's old
        // value never travels, so the last workgroups of a launch end with four posted operations and not
        // with a load round trip (~1 us) on the launch's critical path.  One adder per record and launch,
        // launches in stream order: the sums stay order-deterministic.
        typedef __attribute__((address_space(1))) double gdouble;
        gdouble *q = (gdouble *)p;
        __builtin_amdgcn_global_atomic_fadd_f64(q + 0, v0);
        __builtin_amdgcn_global_atomic_fadd_f64(q + 1, v1);
        __builtin_amdgcn_global_atomic_fadd_f64(q + 2, ta);
        __builtin_amdgcn_global_atomic_fadd_f64(q + 3, th);
    } else { p[0] = v0; p[1] = v1; p[2] = ta; p[3] = th; }
}

// write_partial for a caller that is ONE lane (the 16-wave fp32 wave-tile form's thread 0): the same four values, and
// in accumulate mode the four adds as the hardware instruction itself.  The builtin above goes through the compiler's
// scheme for a wave-uniform address -- count the active lanes, let the first one add value * count -- which with one
// lane active multiplies by 1.0 (the same bits) behind four rounds of v_mbcnt / s_bcnt1 / v_cvt / v_mul / branch, all
// of them between the workgroup's last barrier and the end of the launch.
__device__ __forceinline__ void write_partial_one_lane(double *part, double ta, double th, float inv_scale,
                                                       double inv_rows100, int accum) {
    double *p = part + (size_t)PART_STRIDE * blockIdx.x;
    const double v0 = ta * (double)inv_scale, v1 = th * inv_rows100;
    if (accum) {
        typedef __attribute__((address_space(1))) double gdouble;
        gdouble *q = (gdouble *)p;
        const unsigned zero = 0u;
        asm volatile("global_atomic_add_f64 %0, %1, %2" : : "v"(zero), "v"(v0), "s"(q) : "memory");
        asm volatile("global_atomic_add_f64 %0, %1, %2 offset:8" : : "v"(zero), "v"(v1), "s"(q) : "memory");
        asm volatile("global_atomic_add_f64 %0, %1, %2 offset:16" : : "v"(zero), "v"(ta), "s"(q) : "memory");
        asm volatile("global_atomic_add_f64 %0, %1, %2 offset:24" : : "v"(zero), "v"(th), "s"(q) : "memory");
    } else { p[0] = v0; p[1] = v1; p[2] = ta; p[3] = th; }
}

// A row's term of the batch loss.  A weight of exactly zero takes the row out of the sum whatever its NLL: the
// small-loss baselines and BARE hand their 0/1 selection in as weights, and a row they drop may well have an NLL of
// +inf (its label's class masked to -inf), which 0 * inf would turn into a NaN loss over the rows they kept.
__device__ __forceinline__ float weighted_nll(float li, float pi) { return pi != 0.0f ? li * pi : 0.0f; }

// A row is owned by G consecutive lanes; lane g holds the vectors k*G+g, k < kact <= KMAX, so one
// load instruction reads G*V contiguous elements of each of the wave's 64/G rows and a lane
// amortises the (short) lane-group reductions over up to KMAX*V elements.
template <typename T, int V, int G, int KMAX>
__global__ __launch_bounds__(MSTEP_THREADS) void mstep_kernel(
    const T *__restrict__ logits, int64_t ld, const int64_t *__restrict__ labels,
    const int64_t *__restrict__ idx, int64_t B, int C, int kact, const float *__restrict__ weights,
    int64_t N, float *__restrict__ residuals, float inv_scale,
    const float *__restrict__ grad_scale, T *__restrict__ grad, int64_t ldg, double *__restrict__ part,
    int32_t *__restrict__ status, int accum, double inv_rows100, int64_t first_row) {
    // (argument order = order of first use: what the first row loads need lies in the first 56 bytes, which arrive in
    //  SGPRs at wave start -- rlvi_amd/_build.py: kernarg preload; the same in the other forms below)
    constexpr int R = WAVE / G;  // rows per wave
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int g = lane & (G - 1);
    const int sub = lane / G;
    const float NEG_INF = -__builtin_inff();
    const float gscale = grad_gain(inv_scale, grad_scale);   // the loss, records and residuals never see grad_scale

    float acc = 0.0f;   // sum of pi*l over the rows whose lane-group leader this lane is
    float hits = 0.0f;
    bool bad = false;

    const int64_t stride = (int64_t)gridDim.x * MSTEP_WAVES * R;
    for (int64_t row0 = ((int64_t)blockIdx.x * MSTEP_WAVES + wave) * R; row0 < B; row0 += stride) {
        const int64_t row = row0 + sub;
        const bool valid = row < B;
        const int64_t rr = valid ? row : B - 1;   // padding rows recompute the last row, store nothing
        const T *zrow = logits + rr * ld;

        // Issue order matters: the small label / index reads go FIRST so that they return ahead
        // of the row data (loads of a wave return in order) and the dependent pi gather and
        // label-logit read are already queued while the row vectors are still in flight --
        // otherwise they cost a second full memory round trip behind everybody's row data.
        int64_t y64 = labels[rr];
        int64_t ix = (idx != nullptr ? idx : labels)[rr];   // unconditional load, selected below

        // branch-free row loads: a lane's unused vector slots re-read its first vector (always in
        // range, same cache line) and are masked to -inf afterwards, so the compiler can count
        // the outstanding loads instead of draining them at a branch
        float v[KMAX][V];
        bool live[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int col = (k * G + g) * V;
            live[k] = k < kact && col < C;
            VecIO<T, V>::load(zrow + (live[k] ? col : g * V), v[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
        ix = idx != nullptr ? ix : first_row + rr;    // idx == NULL: identity (in-batch E+M), counted from the batch start
        bool row_ok = valid;
        if (y64 < 0 || y64 >= C) { y64 = 0; bad = bad || valid; row_ok = false; }
        if (ix < 0 || ix >= N) { ix = 0; bad = bad || valid; row_ok = false; }
        const int y = (int)y64;
        const float pi = weights != nullptr ? weights[ix] : 1.0f;   // no weights: plain CE
        // the label logit again (one 4-byte read of a line this wave has just requested)
        float zy;
        {
            float t[1];
            VecIO<T, 1>::load(zrow + y, t);
            zy = t[0];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the two dependent reads queued behind the row data

        float m = NEG_INF;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                v[k][j] = live[k] ? v[k][j] : NEG_INF;
                m = fmaxf(m, v[k][j]);
            }
        m = group_max<G>(m);

        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = mexp(v[k][j] - m);
                v[k][j] = e;
                s += e;
            }
        }
        s = group_sum<G>(s);
        const float logs = logf(s);
        const float li = logs - (zy - m);   // == -((z_y - max) - log(sum exp)), as torch evaluates it

        if (grad != nullptr && valid) {
            const float gs = row_ok ? pi * gscale : 0.0f;   // a rejected row gets a zero gradient row
            const float inv_s = gs / s;
            T *grow = grad + rr * ldg;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int col = (k * G + g) * V;
                if (live[k]) {
                    float o[V];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float p = v[k][j] * inv_s;
                        if (col + j == y) p -= gs;
                        o[j] = p;
                    }
                    VecIO<T, V>::store(grow + col, o);
                }
            }
        }
        // top-1: the label is a hit when it is the FIRST column that attains the row maximum
        // (torch.max order, deep-learning/utils.py:58); two exact maxima put at least 2.0 into the
        // sum, so the exact check (a second read of the row) runs only for waves that hold such a row
        // (!(s < 2): a row of -inf alone has a NaN sum and every column at its maximum -- it takes the check too)
        bool hit = zy == m;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit && !(s < 2.0f)) != 0, 0)) {
            int earlier = 0;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int col = (k * G + g) * V;
                float z[V];
                VecIO<T, V>::load(zrow + (live[k] ? col : g * V), z);
#pragma unroll
                for (int j = 0; j < V; ++j) earlier += (live[k] && z[j] == m && col + j < y) ? 1 : 0;
            }
            earlier = group_allreduce<G>(earlier, FAdd());
            hit = hit && earlier == 0;
        }
        if (g == 0 && row_ok) {
            if (residuals != nullptr) residuals[ix] = li;
            acc += weighted_nll(li, pi);
            hits += hit ? 1.0f : 0.0f;
        }
    }

    // block partials -> workspace (fixed order: deterministic)
    double a = wave_sum((double)acc);
    double h = wave_sum((double)hits);
    __shared__ double sh[2 * MSTEP_WAVES];
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = h; }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, th = 0.0;
#pragma unroll
        for (int w = 0; w < MSTEP_WAVES; ++w) { ta += sh[2 * w]; th += sh[2 * w + 1]; }
        write_partial(part, ta, th, inv_scale, inv_rows100, accum);
    }
}

// ---------------------------------------------------------------------------------------
// Long rows (more than 512 vectors: C > 2048 fp32 / 4096 bf16 aligned, C > 512 in single elements -- an odd
// ImageNet-21k head, a padded pitch): a row does not fit a wave's registers, so ONE WAVE walks its row three times
// from global memory (the second and third pass are L2 hits): maximum -- sum of exponentials, label logit and the
// ties in front of the label -- gradient.  Same arithmetic and the same records as the register-row kernel.
// WPR = waves per row: 1 (a wave per row: many rows) or MSTEP_WAVES (the whole workgroup on one row: batches of
// fewer rows than the chip has wave slots -- 256 x 21 841 is 256 rows).  Four vectors per lane in flight per trip.
template <typename T, int V, int WPR>
__global__ __launch_bounds__(MSTEP_THREADS) void mstep_longrow_kernel(
    const T *__restrict__ logits, int64_t ld, const int64_t *__restrict__ labels,
    const int64_t *__restrict__ idx, int64_t B, int C, int64_t N, const float *__restrict__ weights,
    float *__restrict__ residuals, float inv_scale,
    const float *__restrict__ grad_scale, T *__restrict__ grad, int64_t ldg, double *__restrict__ part,
    int32_t *__restrict__ status, int accum, double inv_rows100) {
    constexpr int U = 4;                                          // vectors per lane and trip
    constexpr int RPB = MSTEP_WAVES / WPR;                        // rows per workgroup at a time
    constexpr int STEP = WPR * WAVE;                              // lanes on one row
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int t = WPR == 1 ? lane : threadIdx.x;                  // this thread's position on its row
    __shared__ float shf[2][MSTEP_WAVES];
    __shared__ int shi[MSTEP_WAVES];
    float acc = 0.0f, hits = 0.0f;
    bool bad = false;
    const float gscale = grad_gain(inv_scale, grad_scale);
    const int nv = C / V;                                         // (V divides C)
    const int64_t stride = (int64_t)gridDim.x * RPB;
    // (every thread of a workgroup runs the same number of trips: the barriers below are uniform)
    for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < B; row0 += stride) {
        const int64_t row = row0 + (WPR == 1 ? wave : 0);
        const bool valid = row < B;
        const int64_t rr = valid ? row : B - 1;                   // a wave without a row recomputes the last one, stores nothing
        const T *zrow = logits + rr * ld;
        int64_t y64 = labels[rr];
        int64_t ix = idx != nullptr ? idx[rr] : rr;
        bool row_ok = valid;
        if (y64 < 0 || y64 >= C) { y64 = 0; bad = bad || valid; row_ok = false; }
        if (ix < 0 || ix >= N) { ix = 0; bad = bad || valid; row_ok = false; }
        const int y = (int)y64;
        const float pi = weights != nullptr ? weights[ix] : 1.0f;
        float zy;
        {
            float tt[1];
            VecIO<T, 1>::load(zrow + y, tt);
            zy = tt[0];
        }
        // ---- pass 1: the row maximum
        float m = -__builtin_inff();
        for (int k0 = t; k0 < nv; k0 += STEP * U) {
            float v[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * STEP;
                VecIO<T, V>::load(zrow + (size_t)(k < nv ? k : k0) * V, v[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) m = fmaxf(m, v[u][j]);      // (a slot past the end repeats k0: harmless for a maximum)
        }
        m = group_max<WAVE>(m);
        if (WPR > 1) {
            if (lane == 0) shf[0][wave] = m;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < MSTEP_WAVES; ++w) m = fmaxf(m, shf[0][w]);
        }
        // ---- pass 2: the sum of exponentials and the ties in front of the label
        float s = 0.0f;
        int earlier = 0;
        for (int k0 = t; k0 < nv; k0 += STEP * U) {
            float v[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * STEP;
                VecIO<T, V>::load(zrow + (size_t)(k < nv ? k : k0) * V, v[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + u * STEP;
                const bool in = k < nv;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    s += in ? mexp(v[u][j] - m) : 0.0f;
                    earlier += (in && v[u][j] == m && k * V + j < y) ? 1 : 0;
                }
            }
        }
        s = group_sum<WAVE>(s);
        earlier = group_allreduce<WAVE>(earlier, FAdd());
        if (WPR > 1) {
            if (lane == 0) { shf[1][wave] = s; shi[wave] = earlier; }
            __syncthreads();
            s = 0.0f;
            earlier = 0;
#pragma unroll
            for (int w = 0; w < MSTEP_WAVES; ++w) { s += shf[1][w]; earlier += shi[w]; }
        }
        const float li = logf(s) - (zy - m);
        // ---- pass 3: the gradient
        if (grad != nullptr && valid) {
            const float gs = row_ok ? pi * gscale : 0.0f;
            const float inv_s = gs / s;
            T *grow = grad + rr * ldg;
            for (int k0 = t; k0 < nv; k0 += STEP * U) {
                float v[U][V];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * STEP;
                    VecIO<T, V>::load(zrow + (size_t)(k < nv ? k : k0) * V, v[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * STEP;
                    if (k < nv) {
                        float o[V];
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            float p = mexp(v[u][j] - m) * inv_s;
                            if (k * V + j == y) p -= gs;
                            o[j] = p;
                        }
                        VecIO<T, V>::store(grow + (size_t)k * V, o);
                    }
                }
            }
        }
        const bool hit = zy == m && earlier == 0;
        if (t == 0 && row_ok) {
            if (residuals != nullptr) residuals[ix] = li;
            acc += weighted_nll(li, pi);
            hits += hit ? 1.0f : 0.0f;
        }
        if (WPR > 1) __syncthreads();                             // (shf / shi are rewritten by the next row)
    }
    double a = wave_sum((double)acc);
    double h = wave_sum((double)hits);
    __shared__ double sh[2 * MSTEP_WAVES];
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = h; }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, th = 0.0;
#pragma unroll
        for (int w = 0; w < MSTEP_WAVES; ++w) { ta += sh[2 * w]; th += sh[2 * w + 1]; }
        write_partial(part, ta, th, inv_scale, inv_rows100, accum);
    }
}

// ---------------------------------------------------------------------------------------
// Wave-tile form (dense rows): every WAVE streams its own tiles of R = 64/G rows through its own
// slice of LDS -- no workgroup barrier anywhere, and the hot loop is straight-line code:
//   A  label / index, then the tile global -> registers -> LDS as flat nontemporal 16-B/lane loads
//      (1 KiB per wave instruction); the pi gather is issued once the tile has landed
//   B  G-lane groups own the rows as in the other forms.  A lane's slots past the end of the row
//      alias the row's LAST vector: they read what its owner reads (harmless for the maximum),
//      are masked out of the sum, and their in-place gradient write repeats the owner's value --
//      no execution-mask juggling.  The -onehot term is one LDS read-modify-write per row (all
//      lanes of the group write the same value)
//   C  flat nontemporal 16-B/lane stores LDS -> grad
// Only full tiles; the launcher hands the B mod R trailing rows to the register-row kernel.
// (Staging the tile by LDS-DMA, global_load_lds_dwordx4, instead of nontemporal register loads + ds_write
// measured slower at 65 536 x 100, 12.3 against 10.4 us: a CU accepts DMA pieces only about as fast as they
// return, so the last workgroup of a CU issues its reads 3 us after the first, while register loads of all
// 16 waves of a CU are in flight at once.)
// ---------------------------------------------------------------------------------------
// -DRLVI_MSTEP_STAMPS: diagnostic build, every wave leaves wall-clock stamps (100 MHz) of its first
// tile's phases in the workspace scratch (tools/mstep_stamps.py); never in the product library.
// Stamp 0 is the wall clock as the kernel's very first instruction (it needs no argument) and stamp 1 the issue of
// the first tile's loads; both wait in registers until the stamp pointer, which hangs on an argument, is there.
#ifdef RLVI_MSTEP_STAMPS
#define RLVI_STAMP(k) do { if (lane == 0 && first_tile) stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RLVI_STAMP(k) do { } while (0)
#endif
constexpr int MSTEP_WAVE_MINW = 4;    // waves per SIMD the register allocation must allow (LDS allows 5)
constexpr int MSTEP_WAVE_WPC = 16;    // waves per CU that stride over the wave tiles

struct FMaxF { __device__ __forceinline__ float operator()(float a, float b) const { return __builtin_fmaxf(a, b); } };

// EXACT: the host guarantees ceil(ceil(C/V)/G) == KMAX, so only a lane's LAST slot can lie past
// the end of the row and (for 16-byte vectors) only the last load / store piece can be partial.
template <typename T, int V, int G, int KMAX, int WPB, bool EXACT>
__global__ __launch_bounds__(WPB *WAVE, MSTEP_WAVE_MINW) void mstep_wave_kernel(
    const T *__restrict__ logits, const int64_t *__restrict__ labels,
    const int64_t *__restrict__ idx, int64_t nfull, int C, int hold_ticks, const float *__restrict__ weights,
    int64_t N, float *__restrict__ residuals, float inv_scale,
    const float *__restrict__ grad_scale, T *__restrict__ grad, double *__restrict__ part,
    int32_t *__restrict__ status, int accum, double inv_rows100, int gen_ticks) {
    // Argument order = order of first use.  logits ... N are the first 56 bytes, preloaded into SGPRs at wave start:
    // the tile grid, the hold's clock and the addresses of the label, index and tile loads need nothing else, so
    // those loads leave without a wait for the argument block; the rest is waited for once, behind them.
#ifdef RLVI_MSTEP_STAMPS
    // The compiler puts its own fetch of the arguments past the preloaded ones at the top of the kernel, in front
    // of anything written here.  So this build does not touch those parameters: it reads them (and the grid size,
    // which the runtime appends to them) from the argument block itself, through a pointer that exists only behind
    // the stamp (offsets = the signature's layout).  NOT the grid size: the runtime appends the hidden arguments only
    // to a kernel whose code asks for them, and a kernel that reads them through this pointer alone has an argument
    // block that ends at gen_ticks -- byte 128 is past it, and a tile loop that advances by whatever lies there does
    // not end when that is zero.  The forms that stride over tiles take gridDim.x as every build does (their entry
    // is not what the stamps are for); the ENTRY_FIRST form has one tile per wave and does not use it.
    unsigned long long t_entry;
    typedef const __attribute__((address_space(4))) char *ms_ka_t;
    ms_ka_t ka = (ms_ka_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("s_memrealtime %0" : "=s"(t_entry));
    asm volatile("" : "+s"(ka));
    __builtin_amdgcn_sched_barrier(0);
#define MS_LATE(U, off) (*(U const __attribute__((address_space(4))) *)(ka + (off)))
    residuals = MS_LATE(float *, 56);
    inv_scale = MS_LATE(float, 64);
    grad_scale = MS_LATE(const float *, 72);
    grad = MS_LATE(T *, 80);
    part = MS_LATE(double *, 88);
    status = MS_LATE(int32_t *, 96);
    accum = MS_LATE(int, 104);
    inv_rows100 = MS_LATE(double, 112);
    gen_ticks = MS_LATE(int, 120);
    const unsigned grid_x = (WPB == 16 && sizeof(T) == 4) ? 0u : gridDim.x;
#undef MS_LATE
#else
    const unsigned grid_x = gridDim.x;
#endif
    constexpr int R = WAVE / G;                                   // rows per wave tile
    constexpr int VB = V * (int)sizeof(T);                        // bytes of a lane vector
    constexpr int NI = (KMAX * VB + 15) / 16;                     // 1-KiB pieces per tile (max)
    constexpr int WTILE = NI * 1024;                              // LDS bytes per wave
    constexpr bool EXACT16 = EXACT && VB == 16;                   // then pieces 0..NI-2 are full
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int g = lane & (G - 1);
    const int sub = lane / G;
    const int nv = C / V;                                         // vectors per row (V divides C)
    const int nchunk = (R * C * (int)sizeof(T)) >> 4;            // 16-byte chunks of a tile
    char *wtile = smem + (size_t)wave * WTILE;
    vu4 *tile16 = reinterpret_cast<vu4 *>(wtile);
    unsigned ngrid = grid_x;
#ifdef RLVI_MSTEP_STAMPS
    bool first_tile = true;
#endif

    // ENTRY_FIRST (the 16-wave fp32 form, one tile per wave: the launch is as long as a wave's own latency): in front
    // of the first tile's loads stands only what their ADDRESSES need, and nothing that hangs on an argument past
    // the preloaded ones.  Every wave of a SIMD issues its prologue before the SIMD's last wave has asked HBM for
    // anything, so an instruction here is paid four times.  The lane's LDS geometry (slot_off, live, row_off), the
    // range checks' constants and the gradient's gain (later arguments and, under a GradScaler, a load) are first
    // used in phase B, behind a wait of microseconds: they are computed behind the issue of the loads and the
    // CU-wide barrier, from copies of lane / wave / C that pass through an empty asm there, so that the compiler
    // cannot hoist them in front of the loop again; the later arguments pass through the same asm.  The other
    // forms keep the gain and the loop invariants in front of the loop: they stride over several tiles or sit at a
    // register bound, where carrying these through the loop costs a register, i.e. a wave per SIMD or a spill.
    constexpr bool ENTRY_FIRST = WPB == 16 && sizeof(T) == 4;

    // loop-invariant per-lane geometry
    // Byte offset of this lane's chunk of piece i, 32 bits: the ENTRY_FIRST form's LOADS take a wave-uniform (scalar)
    // base, this offset and an immediate.  With EXACT16 the pieces 0 .. NI-2 are lane * 16 + i * 1024 -- one register,
    // the piece in the immediate as far as the instruction's offset field reaches -- and only the last one is clamped.
    // (The ENTRY_FIRST form's gradient stores take the same offsets on a scalar base of their own: phase C.  `grad`
    //  passes through the empty asm behind the loads, where the compiler loses its address space, so phase C gives it
    //  a global pointer again; the other forms' stores are flat ones on 64-bit VGPR addresses.)
    unsigned dma_off[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        int c = i * WAVE + lane;
        if (!(EXACT16 && i < NI - 1)) c = c < nchunk ? c : nchunk - 1;   // past the tile: re-read its last chunk
        dma_off[i] = (unsigned)c * 16u;
    }
    int slot_off[KMAX];                                           // LDS byte offset of slot k inside the slice
    bool live[KMAX];
    int row_off = 0;
    // (lane_l, wave_l, C_l: what phases B and C see of the lane, the wave and C; ENTRY_FIRST re-reads them behind the barrier)
    int lane_l = lane, wave_l = wave, C_l = C, g_l = g, sub_l = sub, nv_l = nv;
    char *wtile_l = wtile;
    if constexpr (!ENTRY_FIRST) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int vec = k * G + g;
            live[k] = (EXACT && k < KMAX - 1) || vec < nv;
            slot_off[k] = (sub * C + (live[k] ? vec : nv - 1) * V) * (int)sizeof(T);
        }
        row_off = sub * C * (int)sizeof(T);
    }
    const int64_t *idxp = idx != nullptr ? idx : labels;
    const unsigned sub8 = (unsigned)sub * 8u;
    float gscale = ENTRY_FIRST ? 0.0f : grad_gain(inv_scale, grad_scale);
    bool have_gain = !ENTRY_FIRST;

    float acc = 0.0f, hits = 0.0f;
    bool bad = false;
    // (ENTRY_FIRST: what thread 0 writes the record with.  Thread 0 is in wave 0, and wave 0 of every workgroup has a
    //  tile -- the launcher's grid is exactly ceil(nfull / 16), launch_wave refuses any other -- so the two arguments
    //  are taken on the tile path only, behind the loads; a value that both paths needed would be fetched at the entry)
    int accum_t = 0;
    double inv_rows100_t = 0.0;
    // Reads first, then writes -- chip-wide, without a word exchanged: when every wave of the launch has ONE
    // tile (a launch of up to 16 waves x CUs tiles: the bench block), a wave does not issue its gradient
    // stores before `hold_ticks` x 10 ns after ITS OWN start, the time the launch's reads need at the
    // read-only rate of the memory system.  Until then the tile waits in the wave's LDS slice, finished.
    // Stores that start while other waves' tiles are still landing turn the read stream into a mixed
    // read / write stream (5.4 TB/s instead of 6.5 read-only), and the write burst that follows the read
    // phase is absorbed by the Infinity Cache and drains while the next launch is being dispatched:
    // 11.15 -> 10.5 us per launch at 65 536 x 100 (hold 4.0 us; 3.0 and 6.0 us are both slower than none).
    const unsigned long long t_begin = hold_ticks > 0 ? __builtin_amdgcn_s_memrealtime() : 0ull;

    // CUWIDE (WPB == 16: ONE workgroup per CU, all of its 16 waves): a workgroup barrier right behind the ISSUE
    // of a wave's tile loads -- no wave of the CU sends a store into the CU's memory pipeline before every wave
    // of the CU has its loads in it.  Stamps (tools/mstep_stamps.py) show why that is the moment that counts:
    // the issue of a CU's loads is back-pressured by what the memory system returns -- its last wave issues at
    // 3.6-4.3 us at 65 536 x 100 -- and the first finished waves' stores (from 1.8 us on) queue in front of
    // those loads.  The barrier releases the CU when its last load is in flight: 11.85 -> 10.9 us HBM-cold,
    // 9.5 -> 9.3 us from the Infinity Cache (no estimate of any rate: the data decides), 15.0 -> 13.3 at x 128.
    // (The launcher takes this form only when no wave has a second tile and the grid fills at least four
    //  fifths of the CUs; a wave without a tile only joins the barrier.)
    constexpr bool CUWIDE = WPB == 16;
    // ENTRY_FIRST: ONE tile per wave (the launcher's grid is ceil(nfull / 16) workgroups, at most one per CU), so
    // the tile index and the tile count fit 32 bits: index and compare stay on the scalar unit, and the body
    // leaves after its one pass.
    const int64_t t_first = ENTRY_FIRST ? (int64_t)(blockIdx.x * (unsigned)WPB + (unsigned)wave)
                                        : (int64_t)blockIdx.x * WPB + wave;
    const bool has_tile = ENTRY_FIRST ? (unsigned)t_first < (unsigned)nfull : t_first < nfull;
    if (!ENTRY_FIRST && CUWIDE && !has_tile) __syncthreads();
    for (int64_t t = t_first; ENTRY_FIRST ? has_tile : t < nfull; t += (int64_t)ngrid * WPB) {
        const int64_t row_base = t * R;
        // ---- A
        // (ENTRY_FIRST: 32-bit tile index, C > 0 -- one 32 x 32 -> 64-bit product on the scalar unit)
        const char *src = ENTRY_FIRST
            ? reinterpret_cast<const char *>(logits) + (uint64_t)((unsigned)t * (unsigned)R) * (unsigned)C * sizeof(T)
            : reinterpret_cast<const char *>(logits + row_base * C);
        // label and index first (they return ahead of the tile: loads return in order), the tile's
        // NI chunks per lane behind them
        int64_t y64 = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(labels + row_base) + sub8);
        int64_t ix = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(idxp + row_base) + sub8);
        vu4 stg[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)
            stg[i] = __builtin_nontemporal_load(reinterpret_cast<const vu4 *>(src + dma_off[i]));
#ifdef RLVI_MSTEP_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t_issued = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_sched_barrier(0);
        unsigned long long *stamps = reinterpret_cast<unsigned long long *>(
            reinterpret_cast<char *>(status) + WS_SCRATCH_OFF) + ((size_t)blockIdx.x * WPB + wave) * 16;
        if (lane == 0 && first_tile) {
            stamps[0] = t_entry;
            stamps[1] = t_issued;
            stamps[8] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));     // HW_REG_HW_ID
            stamps[9] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));    // HW_REG_XCC_ID
        }
#endif
        // ENTRY_FIRST: the arguments past the preloaded ones that the body uses pass through here: the compiler asks
        // for them in one burst and waits once, at this point of the program.  (No instruction.)
        // (accum and inv_rows100 are the record's, read by thread 0 behind the last barrier: asked for there they are a
        //  scalar-load round trip at the very end of the launch)
        if constexpr (ENTRY_FIRST) {
            asm volatile("" : "+s"(residuals), "+s"(inv_scale), "+s"(grad_scale), "+s"(grad), "+s"(gen_ticks),
                              "+s"(accum), "+s"(inv_rows100));
            accum_t = accum;
            inv_rows100_t = inv_rows100;
        }
        if (CUWIDE) {
            __builtin_amdgcn_sched_barrier(0);       // (the loads are issued, THEN the barrier)
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        // ENTRY_FIRST: the lane's LDS geometry, while the tile is in flight.  (The asm is empty: it only makes what
        // is derived from the lane, the wave and C depend on this point of the program.)
        if constexpr (ENTRY_FIRST) {
            asm volatile("" : "+v"(lane_l), "+s"(wave_l), "+s"(C_l));
            g_l = lane_l & (G - 1);
            sub_l = (int)((unsigned)lane_l / G);
            nv_l = C_l / V;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {                      // (as in front of the loop, from the copies)
                const int vec = k * G + g_l;
                live[k] = (EXACT && k < KMAX - 1) || vec < nv_l;
                slot_off[k] = (sub_l * C_l + (live[k] ? vec : nv_l - 1) * V) * (int)sizeof(T);
            }
            row_off = sub_l * C_l * (int)sizeof(T);
            wtile_l = smem + (size_t)wave_l * WTILE;
        }
        if constexpr (ENTRY_FIRST) tile16 = reinterpret_cast<vu4 *>(wtile_l);
        if (ENTRY_FIRST && !have_gain) {             // (wave-uniform; behind the barrier)
            gscale = grad_gain(inv_scale, grad_scale);
            have_gain = true;
        }
        bool okrow = true;
        ix = idx != nullptr ? ix : row_base + sub_l;
        if (y64 < 0 || y64 >= C_l) { y64 = 0; okrow = false; }
        if (ix < 0 || ix >= N) { ix = 0; okrow = false; }
        // the tile first, the gather once it has landed: 64 K random 4-byte reads queued beside the
        // streaming reads cost the launch 1 us (12.0 against 11.0 us at 65 536 x 100); issued here they
        // are L2 hits on a quiet queue and fly during the first half of phase B
#pragma unroll
        for (int i = 0; i < NI; ++i) tile16[i * WAVE + lane_l] = stg[i];
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(y64), "+v"(ix) : : "memory");
        float pi = weights != nullptr ? weights[ix] : 1.0f;
        RLVI_STAMP(2);
        bad = bad || !okrow;
        __builtin_amdgcn_wave_barrier();

        // ---- B
        const int y = (int)y64;
        char *zrow = wtile_l + row_off;
        float zy;
        {
            float tt[1];
            VecIO<T, 1>::load(reinterpret_cast<T *>(zrow) + y, tt);
            zy = tt[0];
        }
        float v[KMAX][V];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) VecIO<T, V>::load(reinterpret_cast<T *>(wtile_l + slot_off[k]), v[k]);
        float m = v[0][0];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) m = __builtin_fmaxf(m, v[k][j]);
        m = group_allreduce<G>(m, FMaxF());
#ifdef RLVI_MSTEP_STAMPS
        asm volatile("" : "+v"(m));
        RLVI_STAMP(3);
#endif
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float e = mexp(v[k][j] - m);
                v[k][j] = e;
                s += live[k] ? e : 0.0f;
            }
        s = group_sum<G>(s);
#ifdef RLVI_MSTEP_STAMPS
        asm volatile("" : "+v"(s));
        RLVI_STAMP(4);
#endif
        // s is in [1, C]: v_log_f32 needs no range fix-up
        const float li = __builtin_amdgcn_logf(s) * 0.69314718055994530942f - (zy - m);
        // top-1: the label is a hit when it is the FIRST column that attains the row maximum
        // (torch.max order, deep-learning/utils.py:58).  Two exact maxima put at least 2.0 into
        // the sum, so the exact check runs only for waves that hold such a row.
        pi = okrow ? pi : 0.0f;                                   // a rejected row gets a zero gradient
        bool hit = zy == m;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit && !(s < 2.0f)) != 0, 0)) {
            int earlier = 0;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                float z[V];
                asm volatile("" ::: "memory");                     // re-read, do not keep the first copy live
                VecIO<T, V>::load(reinterpret_cast<T *>(wtile_l + slot_off[k]), z);
                const int col = (k * G + g_l) * V;
#pragma unroll
                for (int j = 0; j < V; ++j) earlier += (live[k] && z[j] == m && col + j < y) ? 1 : 0;
            }
            earlier = group_allreduce<G>(earlier, FAdd());
            hit = hit && earlier == 0;
        }
        if (grad != nullptr) {
            const float gs = pi * gscale;
            const float inv_s = gs * __builtin_amdgcn_rcpf(s);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                float o[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    o[j] = v[k][j] * inv_s;
                    if (sizeof(T) != 4) {
                        const int colc = (live[k] ? (k * G + g_l) : nv_l - 1) * V + j;
                        if (colc == y) o[j] -= gs;
                    }
                }
                VecIO<T, V>::store(reinterpret_cast<T *>(wtile_l + slot_off[k]), o);   // in place
            }
            if (sizeof(T) == 4) {
                // -onehot term: one read-modify-write of the label entry, ordered behind this wave's
                // vector stores (LDS operations of a wave complete in order); the lanes of a group
                // all write the same value
                // (gs = pi * gscale unrounded inside the fma: spelled out so that fused_em.hip,
                //  which promises the same bits, does not depend on what the compiler contracts)
                float *zf = reinterpret_cast<float *>(zrow);
                zf[y] = fmaf(-gscale, pi, zf[y]);
            }
        }
        if constexpr (ENTRY_FIRST) {
            // (a global store: a flat one counts in lgkmcnt as well, out of order, and phase C's LDS reads could
            //  then only be waited for all at once)
            typedef __attribute__((address_space(1))) float gfloat;
            if (g_l == 0 && okrow && residuals != nullptr) ((gfloat *)residuals)[ix] = li;
        } else {
            if (g_l == 0 && okrow && residuals != nullptr) residuals[ix] = li;
        }
        acc += okrow ? weighted_nll(li, pi) : 0.0f;
        hits += (hit && okrow) ? 1.0f : 0.0f;
        __builtin_amdgcn_wave_barrier();
        RLVI_STAMP(5);

        // ---- C: nontemporal store of the gradient tile (flat; ENTRY_FIRST: global)
        if (hold_ticks > 0) {
            while (__builtin_amdgcn_s_memrealtime() - t_begin < (unsigned long long)hold_ticks)
                __builtin_amdgcn_s_sleep(4);
            hold_ticks = gen_ticks > 0 ? hold_ticks + gen_ticks : 0;      // (lab: one hold per generation of tiles)
        }
        if constexpr (ENTRY_FIRST) {
            // ENTRY_FIRST: the gradient through a GLOBAL pointer (behind the pin `grad` is a generic one, and stores
            // through it are flat: 64-bit VGPR addresses, and a count in lgkmcnt that comes back out of order), the
            // tile's base on the scalar unit as the loads' is, and the loads' 32-bit lane offsets.  Global stores leave
            // lgkmcnt to the LDS reads alone, which return in order: piece i leaves when piece i is back and not when
            // piece NI-1 is.  The sched_barriers keep the reads, then the stores, in the order of the pieces.
            if (grad != nullptr) {
                typedef __attribute__((address_space(1))) char gchar;
                typedef __attribute__((address_space(1))) vu4 gvu4;
                gchar *gdst = (gchar *)grad + (uint64_t)((unsigned)t * (unsigned)R) * (unsigned)C * sizeof(T);
                vu4 st[NI];
                unsigned gst_off[NI];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    st[i] = tile16[i * WAVE + lane_l];
                    __builtin_amdgcn_sched_barrier(0);
                    // (empty: the offset's widening to 64 bits has to happen in THIS block for the instruction
                    //  selector to see scalar base + 32-bit offset; the loads' widening is in theirs)
                    // (pieces 1 .. 3 of full pieces: piece 0's register, the piece in the instruction's offset field)
                    if (EXACT16 && i < NI - 1 && i > 0 && i * 1024 < 4096) continue;
                    gst_off[i] = dma_off[i];
                    asm volatile("" : "+v"(gst_off[i]));
                }
                // (nontemporal, as before: sc1 and sc1 nt were measured against it and lost)
#define RLVI_GST(v, o, k) __builtin_nontemporal_store(v, reinterpret_cast<gvu4 *>(gdst + (o) + (k)))
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    if (EXACT16 && i < NI - 1) {
                        if (i > 0 && i * 1024 < 4096) RLVI_GST(st[i], gst_off[0], i * 1024);
                        else RLVI_GST(st[i], gst_off[i], 0);
                    } else if ((i + 1) * WAVE <= nchunk) {
                        RLVI_GST(st[i], gst_off[i], 0);
                    } else if (i * WAVE + lane < nchunk) {
                        RLVI_GST(st[i], gst_off[i], 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
#undef RLVI_GST
            }
        } else if (grad != nullptr) {
            char *gdst = reinterpret_cast<char *>(grad + row_base * C);
            vu4 st[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) st[i] = tile16[i * WAVE + lane_l];    // inside this wave's slice
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (EXACT16 && i < NI - 1) {
                    __builtin_nontemporal_store(st[i], reinterpret_cast<vu4 *>(gdst + dma_off[i]));
                } else if ((i + 1) * WAVE <= nchunk) {
                    __builtin_nontemporal_store(st[i], reinterpret_cast<vu4 *>(gdst + dma_off[i]));
                } else if (i * WAVE + lane < nchunk) {
                    __builtin_nontemporal_store(st[i], reinterpret_cast<vu4 *>(gdst + dma_off[i]));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
#ifdef RLVI_MSTEP_STAMPS
        RLVI_STAMP(6);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        RLVI_STAMP(7);
        first_tile = false;
#endif
        if constexpr (ENTRY_FIRST) break;
    }

    // (ENTRY_FIRST: a wave without a tile joins the barrier of its workgroup's one generation of tiles here, behind
    //  the loop it did not enter, so that its wait for the barrier is not the first thing in the kernel)
    if (ENTRY_FIRST && !has_tile) __syncthreads();
    // every lane of a row's group carried the row's sums: count each row once
    double a = wave_sum((double)(g_l == 0 ? acc : 0.0f));
    // (hits as an integer butterfly, widened once at the end, was measured for the ENTRY_FIRST form and did not show:
    //  profiles/r21_mstep_tail.md)
    double h = wave_sum((double)(g_l == 0 ? hits : 0.0f));
    __shared__ double sh[2 * WPB];
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = h; }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    __syncthreads();
#ifdef RLVI_MSTEP_STAMPS
    // stamps 10 and 11: this wave past the workgroup's last barrier; thread 0 with its record's four adds issued
    unsigned long long *stamps_end = reinterpret_cast<unsigned long long *>(
        reinterpret_cast<char *>(status) + WS_SCRATCH_OFF) + ((size_t)blockIdx.x * WPB + wave) * 16;
    if (lane == 0) stamps_end[10] = __builtin_amdgcn_s_memrealtime();
#endif
    if (threadIdx.x == 0) {
        double ta = 0.0, th = 0.0;
        if constexpr (ENTRY_FIRST) {
            // ENTRY_FIRST: the launch ends when the slowest CU's thread 0 is through here.  All sixteen pairs are asked
            // for before the first add (one LDS round trip, not eight); the sums keep their order, w = 0 .. WPB-1.
            // (The last pair is asked for behind the first two adds, into registers they have freed: sixteen pairs at
            //  once are 64 registers, and with the address the kernel would be past 64, a wave per SIMD on paper.)
            double s[2 * WPB];
#pragma unroll
            for (int w = 0; w < 2 * WPB - 2; ++w) s[w] = sh[w];
            __builtin_amdgcn_sched_barrier(0);
            ta += s[0]; th += s[1];
            ta += s[2]; th += s[3];
            __builtin_amdgcn_sched_barrier(0);
            s[2 * WPB - 2] = sh[2 * WPB - 2]; s[2 * WPB - 1] = sh[2 * WPB - 1];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int w = 2; w < WPB; ++w) { ta += s[2 * w]; th += s[2 * w + 1]; }
            write_partial_one_lane(part, ta, th, inv_scale, inv_rows100_t, accum_t);
        } else {
#pragma unroll
            for (int w = 0; w < WPB; ++w) { ta += sh[2 * w]; th += sh[2 * w + 1]; }
            write_partial(part, ta, th, inv_scale, inv_rows100, accum);
        }
#ifdef RLVI_MSTEP_STAMPS
        stamps_end[11] = __builtin_amdgcn_s_memrealtime();
#endif
    }
}

// ---------------------------------------------------------------------------------------
// bf16 / fp16 rows of an ODD number of elements (C = 101: 202-byte rows, every other row starts in the
// middle of a 32-bit word), at least 32 768 of them (round 4; the round-3 verdict's item 4b).  The general wave tile
// reads such a row one 2-byte element per LDS instruction (27.5 us at 65 536 x 101, so the launcher sent the shape
// to the register-row kernel: 14.3 us).  Here the tile is the same flat 16-B/lane stream into LDS, but a lane owns a
// CONTIGUOUS segment of its row -- four lanes per row, L = ceil(C / 4) elements each -- and reads it as 32-bit words
// from the word its first element lies in; v_alignbit re-aligns the words of an odd start, a shift and a mask widen the
// two halves (Half<T>: bf16 or fp16).  The gradient goes back in place as 2-byte halves (v_cvt_pk_bf16_f32 or
// v_cvt_pk_f16_f32 per pair, one 16-bit LDS store per element: a word of the tile may belong to two lanes, or two
// rows) and leaves as flat 16-B stores.
// ---------------------------------------------------------------------------------------
template <typename T, int KW, int WPB>
__global__ __launch_bounds__(WPB *WAVE, 4) void mstep_bf16w_kernel(
    const T *__restrict__ logits, const int64_t *__restrict__ labels, const int64_t *__restrict__ idx,
    int64_t nfull, int C, const float *__restrict__ weights, int64_t N, float *__restrict__ residuals,
    float inv_scale, const float *__restrict__ grad_scale, T *__restrict__ grad, double *__restrict__ part,
    int32_t *__restrict__ status, int accum, double inv_rows100) {
    static_assert(sizeof(T) == 2, "word-wise tile of 2-byte elements");
    constexpr int R = 16, G = 4, NI = 4;                          // 16 rows x <= 128 elements x 2 B <= 4 KiB
    constexpr int WTILE = NI * 1024 + 64;                         // (+ a pad: the word past a segment's end, dummy stores)
    constexpr int NE = 2 * KW;                                    // element slots of a lane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int g = lane & (G - 1), sub = lane / G;
    char *wtile = smem + (size_t)wave * WTILE;
    vu4 *tile16 = reinterpret_cast<vu4 *>(wtile);
    const int nchunk = 2 * C;                                     // 16-byte chunks of a tile (16 rows x 2 C bytes)
    const int L = (C + 3) >> 2;
    const int e0 = g * L;
    const int cnt = C - e0 < L ? (C - e0 > 0 ? C - e0 : 0) : L;   // elements of this lane's segment
    const int E0 = sub * C + e0;                                  // first element, counted in the tile
    const unsigned shift = (unsigned)(E0 & 1) * 16u;              // odd start: the segment begins in a word's high half
    const int W0 = E0 >> 1;
    const int64_t *idxp = idx != nullptr ? idx : labels;
    const unsigned sub8 = (unsigned)sub * 8u;
    const int64_t tstride = (int64_t)gridDim.x * WPB;
    const float gscale = grad_gain(inv_scale, grad_scale);
    float acc = 0.0f, hits = 0.0f;
    bool bad = false;
    for (int64_t t = (int64_t)blockIdx.x * WPB + wave; t < nfull; t += tstride) {
        const int64_t row_base = t * R;
        const char *src = reinterpret_cast<const char *>(logits + row_base * C);
        int64_t y64 = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(labels + row_base) + sub8);
        int64_t ix = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(idxp + row_base) + sub8);
        vu4 stg[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            int c = i * WAVE + lane;
            c = c < nchunk ? c : nchunk - 1;                      // past the tile: re-read its last chunk
            stg[i] = __builtin_nontemporal_load(reinterpret_cast<const vu4 *>(src + (size_t)c * 16));
        }
        bool okrow = true;
        ix = idx != nullptr ? ix : row_base + sub;
        if (y64 < 0 || y64 >= C) { y64 = 0; okrow = false; }
        if (ix < 0 || ix >= N) { ix = 0; okrow = false; }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (i * WAVE + lane < nchunk) tile16[i * WAVE + lane] = stg[i];
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(y64), "+v"(ix) : : "memory");
        float pi = weights != nullptr ? weights[ix] : 1.0f;         // behind the tile (see mstep_wave_kernel)
        bad = bad || !okrow;
        __builtin_amdgcn_wave_barrier();

        // ---- B: the segment as words, re-aligned, widened
        const int y = (int)y64;
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(wtile);
        const uint16_t *h16 = reinterpret_cast<const uint16_t *>(wtile);
        const float zy = Half<T>::widen(h16[sub * C + y]);
        uint32_t w[KW + 1];
#pragma unroll
        for (int k = 0; k <= KW; ++k) w[k] = w32[W0 + k];
        float v[NE];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const uint32_t x = __builtin_amdgcn_alignbit(w[k + 1], w[k], shift);      // elements 2k, 2k + 1
            v[2 * k] = Half<T>::lo(x);
            v[2 * k + 1] = Half<T>::hi(x);
        }
        const float NEG_INF = -__builtin_inff();
        float m = NEG_INF;
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            v[j] = j < cnt ? v[j] : NEG_INF;
            m = __builtin_fmaxf(m, v[j]);
        }
        m = group_allreduce<G>(m, FMaxF());
        const bool hit0 = zy == m;
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            v[j] = mexp(v[j] - m);                                // a slot past the segment: exp(-inf) = 0
            s += v[j];
        }
        s = group_sum<G>(s);
        const float li = __builtin_amdgcn_logf(s) * 0.69314718055994530942f - (zy - m);
        pi = okrow ? pi : 0.0f;
        // top-1: the label is a hit when it is the FIRST column that attains the row maximum; two exact maxima put
        // at least 2.0 into the sum, so the exact check (the words are still in registers) runs only for waves
        // that hold such a row
        bool hit = hit0;
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit0 && !(s < 2.0f)) != 0, 0)) {
            int earlier = 0;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const uint32_t x = __builtin_amdgcn_alignbit(w[k + 1], w[k], shift);
                const float z0 = Half<T>::lo(x), z1 = Half<T>::hi(x);
                earlier += (2 * k < cnt && z0 == m && e0 + 2 * k < y) ? 1 : 0;
                earlier += (2 * k + 1 < cnt && z1 == m && e0 + 2 * k + 1 < y) ? 1 : 0;
            }
            hit = hit0 && group_allreduce<G>(earlier, FAdd()) == 0;
        }
        if (grad != nullptr) {
            const float gs = pi * gscale;
            const float inv_s = gs * __builtin_amdgcn_rcpf(s);
            const int jy = y - e0;                                // the label's slot, if it lies in this segment
            uint16_t *o16 = reinterpret_cast<uint16_t *>(wtile);
            const int dummy = NI * 512 + (lane & 15);             // a halfword of the pad, per lane
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                float o0 = v[2 * k] * inv_s, o1 = v[2 * k + 1] * inv_s;
                o0 = 2 * k == jy ? o0 - gs : o0;
                o1 = 2 * k + 1 == jy ? o1 - gs : o1;
                const uint32_t pk = Half<T>::narrow2(o0, o1);
                o16[2 * k < cnt ? E0 + 2 * k : dummy] = (uint16_t)(pk & 0xFFFFu);
                o16[2 * k + 1 < cnt ? E0 + 2 * k + 1 : dummy] = (uint16_t)(pk >> 16);
            }
        }
        if (g == 0 && okrow && residuals != nullptr) residuals[ix] = li;
        acc += okrow ? weighted_nll(li, pi) : 0.0f;
        hits += (hit && okrow) ? 1.0f : 0.0f;
        __builtin_amdgcn_wave_barrier();

        // ---- C: flat store of the gradient tile
        if (grad != nullptr) {
            char *gdst = reinterpret_cast<char *>(grad + row_base * C);
            vu4 st[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) st[i] = tile16[(i * WAVE + lane < nchunk) ? i * WAVE + lane : 0];
#pragma unroll
            for (int i = 0; i < NI; ++i)
                if (i * WAVE + lane < nchunk)
                    __builtin_nontemporal_store(st[i], reinterpret_cast<vu4 *>(gdst + (size_t)(i * WAVE + lane) * 16));
        }
        __builtin_amdgcn_wave_barrier();
    }
    double a = wave_sum((double)(g == 0 ? acc : 0.0f));
    double h = wave_sum((double)(g == 0 ? hits : 0.0f));
    __shared__ double sh[2 * WPB];
    if (lane == 0) { sh[2 * wave] = a; sh[2 * wave + 1] = h; }
    if (bad) atomicOr(status, RLVI_ST_RANGE);
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, th = 0.0;
#pragma unroll
        for (int w = 0; w < WPB; ++w) { ta += sh[2 * w]; th += sh[2 * w + 1]; }
        write_partial(part, ta, th, inv_scale, inv_rows100, accum);
    }
}

// Hold of the reads-then-writes form for a launch that reads `bytes` of logits, in ticks of 10 ns: the time
// its reads need at the read-only rate.  Fitted to the best hold of a sweep per shape (tools/sweep_hold.sh:
// 13.6 MB bf16 -> 2.4 us, 16.8 MB -> 2.9, 19.7 MB -> 3.4, 26.2 MB -> 4.3, 33.5 MB -> 5.2): 0.68 us of ramp-up
// + bytes / 7.25 TB/s; within +-0.3 us of the best hold most of the gain stays, 1 us off is worse than
// none.  Below 12 MB no hold was found to help (the launch is over before the phases could separate).
static inline int mstep_hold_ticks(double bytes) {
    if (bytes < 12.0e6) return 0;
    return (int)((0.68 + bytes / 7.25e6) * 100.0);
}

__global__ __launch_bounds__(256) void mstep_finalize_kernel(double *__restrict__ part, int nblocks,
                                                             double scale, float *__restrict__ out,
                                                             int clear) {
    reduce_partials(part, nblocks, scale, out, clear != 0, 256);
}

// The launcher's knobs (tests and the committed sweep scripts set them), read once per call.
struct MstepKnobs {
    int form;        // RLVI_MSTEP_FORM: see launch_mstep
    int force_g;     // RLVI_MSTEP_G: lanes per row, 0 = the dispatch rules decide
    int cuwide;      // RLVI_MSTEP_CUWIDE: the 16-wave barrier form where its conditions hold
    int hold, gen;   // RLVI_MSTEP_HOLD, RLVI_MSTEP_GEN: see launch_mstep
};

// One M-step call: the caller's (checked) arguments and what every form derives from them, filled once by
// mstep_entry and handed down by reference.
template <typename T>
struct MstepCall {
    const T *logits;
    int64_t ld;
    const int64_t *labels, *idx;
    const float *weights;
    float *residuals;
    int64_t N, B;
    int C;
    float inv_scale;
    const float *grad_scale;
    T *grad;
    int64_t ldg;
    float *out;
    void *ws;
    hipStream_t st;
    MstepKnobs knobs;
    // (a call with `out` has records of its own: it never touches what an accumulate sequence has piled up)
    double *part;
    int32_t *status;
    int accum;                // no `out`: accumulate for rlvi_epoch_end_f32
    double inv_rows100;
    int cus;

    // Workgroups of `wpb` waves for `tiles` wave tiles: MSTEP_WAVE_WPC waves per CU stride over the tiles (one tile each
    // at the bench size), and every workgroup owns a record
    int64_t tile_grid(int64_t tiles, int wpb) const {
        int64_t nb = (tiles + wpb - 1) / wpb;
        int64_t cap = ((int64_t)MSTEP_WAVE_WPC * cus + wpb - 1) / wpb;
        if (cap > MSTEP_MAX_BLOCKS) cap = MSTEP_MAX_BLOCKS;
        return nb > cap ? cap : nb;
    }
    // The register-row kernel over the rows from `first` on, in `nb` workgroups.  Behind a tile form (first > 0):
    // the trailing rows, one workgroup adding to record 0
    template <int V, int G, int KMAX>
    int rows(int64_t first, int64_t nb) const {
        const int kact = ((C + V - 1) / V + G - 1) / G;
        return launch(mstep_kernel<T, V, G, KMAX>, dim3((unsigned)nb), dim3(MSTEP_THREADS), 0, st,
                      logits + first * ld, ld, labels + first, idx != nullptr ? idx + first : idx, B - first, C, kact,
                      weights, N, residuals, inv_scale, grad_scale,
                      grad != nullptr ? grad + first * ldg : grad, ldg, part, status, first > 0 ? 1 : accum,
                      inv_rows100, first);
    }
    // What follows a tile form's launch (rc) over `done` rows in `nb` workgroups: the trailing rows, then as finish()
    template <int V, int G, int KMAX>
    int tail_and_finish(int rc, int64_t done, int64_t nb) const {
        if (rc == 0 && done < B) rc = rows<V, G, KMAX>(done, 1);
        return finish(rc, nb);
    }
    // The caller's `out` from the `nb` records of the launch (rc) before
    int finish(int rc, int64_t nb) const {
        if (rc != 0 || out == nullptr) return rc;
        // the finalize pass clears what it read: records are all-zero outside an accumulate sequence
        return launch(mstep_finalize_kernel, dim3(1), dim3(256), 0, st, part, (int)nb, 1.0, out, 1);
    }
};

// mstep_wave_kernel<T, V, G, KMAX, WPB, exact> over `nfull` tiles in `nb` workgroups
template <typename T, int V, int G, int KMAX, int WPB>
static int launch_wave(const MstepCall<T> &c, bool exact, int64_t nb, int64_t nfull, int hold_ticks, int gen_ticks) {
    constexpr size_t LDS = (size_t)WPB * ((KMAX * V * sizeof(T) + 15) / 16) * 1024;
    // (the kernel's ENTRY_FIRST form does not stride: a grid that left a wave a second tile would drop it)
    // (nor one with a workgroup that has no tile at all: its thread 0 writes the record from what wave 0's tile path left)
    if (WPB == 16 && sizeof(T) == 4 && (nfull > nb * WPB || nfull <= (nb - 1) * WPB)) return RLVI_E_LIMIT;
    auto go = [&](auto kern) {
        if constexpr (WPB == 16) {      // (> 64 KiB of dynamic LDS)
            if (const int e = allow_dyn_lds(kern, LDS)) return e;
        }
        return launch(kern, dim3((unsigned)nb), dim3(WPB * WAVE), LDS, c.st, c.logits, c.labels, c.idx, nfull, c.C,
                      hold_ticks, c.weights, c.N, c.residuals, c.inv_scale, c.grad_scale, c.grad, c.part, c.status,
                      c.accum, c.inv_rows100, gen_ticks);
    };
    return exact ? go(mstep_wave_kernel<T, V, G, KMAX, WPB, true>) : go(mstep_wave_kernel<T, V, G, KMAX, WPB, false>);
}

template <typename T, int V, int G, int KMAX>
static int launch_mstep(const MstepCall<T> &c) {
    constexpr int R = WAVE / G;
    constexpr int WPB = 4;                          // waves per workgroup of the wave-tile form
    const int64_t B = c.B;
    const int C = c.C;
    // form: 1 = wave tiles through LDS (dense rows), 0 = register rows everywhere; -1 (default): wave tiles
    // once the launch has more than two waves per CU (512 tiles) -- below that a call is one wave's latency
    // long, and global -> registers -> global is shorter than the trip through LDS (tools/sweep_small.sh:
    // 4096 x 10 3.4 -> 3.1 us, 4096 x 100 4.05 -> 3.7; 16 384 x 100 the other way, 5.2 against 5.7)
    int form = c.knobs.form;
    if (form < 0) form = (B + R - 1) / R > 512 ? 1 : 0;
    const bool flat16 = c.ld == C && (c.grad == nullptr || c.ldg == C) &&
                        ((uintptr_t)c.logits % 16) == 0 && ((uintptr_t)c.grad % 16) == 0;
    const size_t wtile_bytes = (size_t)R * C * sizeof(T);
    constexpr size_t SKB = (size_t)((KMAX * V * sizeof(T) + 15) / 16);
    const bool dense_wave = flat16 && wtile_bytes % 16 == 0 && wtile_bytes / 16 <= SKB * WAVE;
    const int64_t nfull = B / R;
    if (!(dense_wave && form >= 1 && nfull > 0)) {
        const int64_t rows_per_block = (int64_t)MSTEP_WAVES * R;
        int64_t nb = (B + rows_per_block - 1) / rows_per_block;
        if (nb > MSTEP_MAX_BLOCKS) nb = MSTEP_MAX_BLOCKS;
        if (nb < 1) nb = 1;
        ws_note_mstep(c.ws, 1, V, G, KMAX);
        return c.finish(c.template rows<V, G, KMAX>(0, nb), nb);
    }
    // (extra LDS per workgroup -- fewer resident workgroups per CU, the dispatcher then hands the remaining tiles
    //  to whichever CU frees up first -- measured slower: DESIGN.md 3.1)
    int64_t nb = c.tile_grid(nfull, WPB);
    // reads-then-writes hold (see the kernel): only when no wave has a second tile and a gradient is
    // written.  RLVI_MSTEP_HOLD = ticks of 10 ns; 0 (the default): off; -1: from the bytes the launch
    // reads AT THE HBM READ RATE -- for logits that stream from HBM (a block that is not resident in the
    // Infinity Cache: bench.py's rotation of twelve blocks, a block larger than the cache).  Logits that
    // the model's last layer has just written are served by the cache, their read phase is over sooner
    // than the hold assumes, and the hold then COSTS time (single buffer pair: 9.4 -> 10.3 us): the
    // caller knows which case it is in, the kernel does not (a per-CU barrier between reads and writes
    // -- 16-wave workgroups -- was built to let the data decide: no gain cold, 9.4 -> 10.1 us warm).
    // (the caller's hint lives with the caller's workspace -- rlvi_workspace_set_option(ws, "logits_from_hbm", 1)
    //  -- not with the process: two training loops, or two streams, do not see each other's; the knob of the
    //  same meaning is the lab override)
    int hold_ticks = c.knobs.hold;
    int gen_ticks = c.knobs.gen;      // ticks between the holds of successive tile generations
    const int64_t waves = nb * WPB;
    const double gen_bytes = (double)(nfull < waves ? nfull : waves) * (double)wtile_bytes;
    if (nfull > waves && hold_ticks < 0 && gen_ticks < 0) {
        // several tiles per wave under the caller's HBM hint: one hold per GENERATION of tiles, the
        // generations one read + one write of their bytes at the mixed rate apart (2 x 26.2 MB: 9.0 us).
        // Only where it was measured to pay (tools/sweep_gen.sh): fp32, two to four FULL generations
        // (65 536 x 100 per generation: 21.8 -> 20.0 us at two, 30.6 -> 29.3 at three, 39.8 -> 39.0 at four;
        // five gain or lose a per cent with the spacing, a half-filled last generation or eight lose)
        const int64_t gens = nfull / waves;
        gen_ticks = (sizeof(T) == 4 && nfull % waves == 0 && gens >= 2 && gens <= 4 && gen_bytes >= 12.0e6)
                        ? (int)(2.0 * gen_bytes / 5.76e6 * 100.0) : 0;
    }
    if (gen_ticks < 0) gen_ticks = 0;
    if (c.grad == nullptr || (nfull > waves && gen_ticks <= 0 && hold_ticks < 0)) hold_ticks = 0;
    if (hold_ticks < 0) hold_ticks = mstep_hold_ticks(gen_bytes);
    if (hold_ticks == 0) gen_ticks = 0;
    const bool exact = ((C + V - 1) / V + G - 1) / G == KMAX;
    int rc = 0;
    bool cuwide = false;
    if constexpr (G == 4 && V * sizeof(T) == 16) {
        constexpr int WPB16 = 16;
        const int64_t nb16 = (nfull + WPB16 - 1) / WPB16;
        // (a caller that has hinted HBM-resident logits gets the four-wave workgroups with the timed hold:
        //  10.65 against 10.95 us -- the timed hold separates the phases chip-wide, the barrier per CU)
        cuwide = c.knobs.cuwide && c.grad != nullptr && hold_ticks == 0 && nb16 <= c.cus &&
                 nb16 * 5 >= (int64_t)c.cus * 4 && nb16 <= MSTEP_MAX_BLOCKS;
        if (cuwide) {
            // (nb16 workgroups of 16 waves = ONE tile per wave, never a capped grid: the fp32 kernel of this form
            //  relies on it -- 32-bit tile index, one pass through its body, no stride)
            nb = nb16;
            ws_note_mstep(c.ws, 3, V, G, KMAX);
            rc = launch_wave<T, V, G, KMAX, WPB16>(c, exact, nb, nfull, 0, 0);
        }
    }
    if (!cuwide) {
        ws_note_mstep(c.ws, 2 + (hold_ticks != 0 ? 16 : 0), V, G, KMAX);
        rc = launch_wave<T, V, G, KMAX, WPB>(c, exact, nb, nfull, hold_ticks, gen_ticks);
    }
    return c.template tail_and_finish<V, G, KMAX>(rc, nfull * R, nb);
}

// Picks the lane group: the smallest G whose lanes need at most 8 vectors each (so the short
// DPP reductions are amortised over up to 8*V elements per lane); rows of <= 8 vectors are
// handled by a single lane.
template <typename T, int V>
static int dispatch_gk(const MstepCall<T> &c) {
    const int64_t B = c.B;
    const int C = c.C;
    const int nv = (C + V - 1) / V;
    const int force_g = c.knobs.force_g;
#define RLVI_CASE(G_, K_) return launch_mstep<T, V, G_, K_>(c)
    // (bf16 in 16-byte vectors: at most FOUR vectors = 32 elements per lane, as fp32's eight -- with 64 elements a lane's
    //  serial work and its registers cost more than the shorter reductions save: tools/lab/sweep_g_bf16.sh, 16 384 x 256
    //  11.2 -> 6.5 us, x 512 15.8 -> 8.6, x 1000 24.3 -> 15.8, x 2000 39.5 -> 26.7, 4096 x 1000 10.8 -> 6.6)
    //  Rows of up to 20 vectors keep the 16-row tile with four lanes per row: five vectors per lane there beat three on
    //  eight lanes, 65 536 x 136 10.6 against 13.3 us, x 160 11.1 against 13.7; x 200 -- seven -- 15.7 against 14.4.)
    constexpr bool WIDE_BF16 = sizeof(T) == 2 && V == 8;
    const int kpref = (WIDE_BF16 && nv > 20) ? 4 : 8;
    int gsel = 64;
    for (int gg = 1; gg <= 64; gg <<= 1)
        if ((nv + gg - 1) / gg <= kpref) { gsel = gg; break; }
    // 64-row tiles (G = 4) measured best whenever a row has at least 8 vectors (fp32 C = 100:
    // 10.8 us against 11.8 for G = 8; bf16 C = 104: 8.7 us against 12.3 for G = 2)
    if (gsel < 4 && nv >= 8) gsel = 4;
    if (force_g && (nv + force_g - 1) / force_g <= 8) gsel = force_g;
    // rows of up to 128 elements whose length is not a multiple of the 16-byte vector (C = 101:
    // V = 1) keep the 64-row tile and four lanes per row, each lane holding up to 32 / V short
    // vectors: 11.6 us instead of 20.0 at 65 536 x 101 fp32 (the 16-lane form spends its time in
    // per-element address arithmetic and DPP steps)
    // -- only for launches of at least two such tiles per SIMD (fp32 C = 101: 8.6 against 9.4 us at 32 768
    // rows, 7.2 against 5.8 at 16 384, 5.7 against 3.1 at 1024), and never for single 2-byte elements (bf16
    // C = 101: one ds_read_u16 per element, 27.5 against 14.3 us at 65 536 rows, 9.2 against 3.1 at 1024)
    if constexpr (V * sizeof(T) < 16 && V * sizeof(T) > 2) {
        if (gsel > 4 && C <= 128 && !force_g && B >= 16 * 2048) {
            const int k4 = (nv + 3) / 4;
            if (k4 <= 16) RLVI_CASE(4, 16);
            if constexpr (V == 1) RLVI_CASE(4, 32);
        }
        // the same for rows of 129 ... 512 such elements (Places365's 365 classes): sixteen lanes per row, four rows per
        // wave tile, instead of one row per wave in single 4-byte loads
        // -- 65 536 x 365 fp32 46.0 -> 39.5 us, 16 384 x 365 15.5 -> 11.8, 65 536 x 201 27.9 -> 22.1, 65 536 x 366 bf16
        // 30.9 -> 24.4; not below 8192 rows (4096 x 365: 5.9 against 7.2) and not beyond 24 single elements per lane (x 511:
        // 54.6 against 58.0, the 32-slot form spills)
        if (gsel > 16 && C > 128 && C <= 512 && !force_g && B >= 8192) {
            const int k16 = (nv + 15) / 16;
            if constexpr (!(sizeof(T) == 2 && V == 4)) {         // (bf16 in 8-byte vectors never has gsel > 16 here)
                if (k16 <= 16) RLVI_CASE(16, 16);
            }
            if constexpr (V == 1) {
                if (k16 <= 24) RLVI_CASE(16, 24);
            }
        }
    }
    // a launch of less than one wave per SIMD is as long as ONE wave's instruction stream (a lone wave issues
    // an instruction every ~6 clocks): twice the lanes per row halve it (tools/sweep_small.sh: 4096 x 10
    // 3.65 -> 3.3 us, 4096 x 100 4.4 -> 4.05, 1024 x 101 3.35 -> 3.1; from 1024 waves on the wider tile wins)
    if (!force_g && kpref == 8 && gsel < 64 && (nv + gsel - 1) / gsel >= 2 && (B * gsel + 63) / 64 < 1024) gsel *= 2;
    // bf16 rows of five to eight 16-byte vectors (C = 40 ... 64) from 16 384 rows on: two lanes per row (32 rows per wave
    // tile) -- 65 536 x 64 8.6 -> 7.1 us, x 48 10.6 -> 7.0, x 40 10.5 -> 6.8, 262 144 x 64 22.5 -> 18.2; nine vectors (x 72) are
    // better off with four lanes, four (x 32) with one.  (fp32 C = 20 ... 32 would gain 8-12 % too -- 65 536 x 32 6.75 -> 6.2 us --
    // but the one-launch in-batch E+M promises the bits of this kernel's four-lane row sums at those shapes.)
    if (!force_g && sizeof(T) == 2 && V == 8 && nv >= 5 && nv <= 8 && B >= 16384) gsel = 2;
    const int k = (nv + gsel - 1) / gsel;
    if (k > 8) {
        // more than 512 vectors per row: a wave (or, for few rows, a workgroup) per row, three passes (mstep_longrow_kernel)
        // fewer rows than four per CU: the whole workgroup on one row
        const bool wide = B <= 4 * (int64_t)c.cus;
        int64_t nb = wide ? B : (B + MSTEP_WAVES - 1) / MSTEP_WAVES;
        if (nb > MSTEP_MAX_BLOCKS) nb = MSTEP_MAX_BLOCKS;
        ws_note_mstep(c.ws, 5, V, 0, 0);
        auto go = [&](auto kern) {
            return launch(kern, dim3((unsigned)nb), dim3(MSTEP_THREADS), 0, c.st, c.logits, c.ld, c.labels, c.idx,
                          B, C, c.N, c.weights, c.residuals, c.inv_scale, c.grad_scale, c.grad, c.ldg, c.part, c.status,
                          c.accum, c.inv_rows100);
        };
        return c.finish(wide ? go(mstep_longrow_kernel<T, V, MSTEP_WAVES>) : go(mstep_longrow_kernel<T, V, 1>), nb);
    }
    switch (gsel) {
        case 1:
            if (k <= 1) RLVI_CASE(1, 1);
            if (k <= 2) RLVI_CASE(1, 2);
            if (k <= 4) RLVI_CASE(1, 4);
            RLVI_CASE(1, 8);
        case 2: if (k <= 4) RLVI_CASE(2, 4); RLVI_CASE(2, 8);
        case 4:
            if (k <= 4) RLVI_CASE(4, 4);
            if (k == 5) RLVI_CASE(4, 5);
            if (k == 6) RLVI_CASE(4, 6);
            if (k == 7) RLVI_CASE(4, 7);
            RLVI_CASE(4, 8);
        case 8: if (k <= 2) RLVI_CASE(8, 2); if (k <= 4) RLVI_CASE(8, 4); RLVI_CASE(8, 8);
        case 16: if (k <= 4) RLVI_CASE(16, 4); RLVI_CASE(16, 8);
        case 32: if (k <= 4) RLVI_CASE(32, 4); RLVI_CASE(32, 8);
        default: if (k <= 4) RLVI_CASE(64, 4); RLVI_CASE(64, 8);
    }
#undef RLVI_CASE
}

// The word-wise wave tile (mstep_bf16w_kernel); the B mod 16 trailing rows go to the register-row kernel.
template <typename T>
static int launch_bf16w(const MstepCall<T> &c) {
    constexpr int WPB = 4;
    const int64_t nfull = c.B / 16;
    const int64_t nb = c.tile_grid(nfull, WPB);
    const size_t lds = (size_t)WPB * (4 * 1024 + 64);
    const int kw = ((c.C + 3) / 4 + 1) / 2;        // words of a lane's segment of ceil(C / 4) elements
    ws_note_mstep(c.ws, 4, 1, 0, 0);
    auto go = [&](auto kern) {
        return launch(kern, dim3((unsigned)nb), dim3(WPB * WAVE), lds, c.st, c.logits, c.labels, c.idx, nfull, c.C,
                      c.weights, c.N, c.residuals, c.inv_scale, c.grad_scale, c.grad, c.part, c.status, c.accum,
                      c.inv_rows100);
    };
    const int rc = kw <= 8    ? go(mstep_bf16w_kernel<T, 8, WPB>)
                   : kw <= 13 ? go(mstep_bf16w_kernel<T, 13, WPB>)
                              : go(mstep_bf16w_kernel<T, 16, WPB>);
    return c.template tail_and_finish<1, 16, 8>(rc, nfull * 16, nb);
}

template <typename T>
static int mstep_entry(const T *logits, int64_t ld, const int64_t *labels, const int64_t *idx,
                       const float *weights, float *residuals, int64_t N, int64_t B, int64_t C,
                       float inv_scale, const float *grad_scale, T *grad, int64_t ldg, float *out, void *ws,
                       void *stream) {
    if (!logits || !labels || !ws) return RLVI_E_NULL;
    if (!weights && idx) return RLVI_E_NULL;       // an index without the vector it indexes
    if (!weights) N = B;                            // evaluation form: identity rows, pi = 1
    if (B <= 0 || C <= 0 || N <= 0 || ld < C || (grad && ldg < C)) return RLVI_E_SHAPE;
    if (C > (1 << 20)) return RLVI_E_LIMIT;
    if (((uintptr_t)labels & 7) || ((uintptr_t)idx & 7) || ((uintptr_t)weights & 3) ||
        ((uintptr_t)residuals & 3) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 255) || ((uintptr_t)grad_scale & 3) ||
        ((uintptr_t)logits % sizeof(T)) || (grad && ((uintptr_t)grad % sizeof(T))))
        return RLVI_E_ALIGN;
    char *base = static_cast<char *>(ws);
    MstepCall<T> c;
    c.logits = logits; c.ld = ld; c.labels = labels; c.idx = idx; c.weights = weights; c.residuals = residuals;
    c.N = N; c.B = B; c.C = (int)C; c.inv_scale = inv_scale; c.grad_scale = grad_scale; c.grad = grad; c.ldg = ldg;
    c.out = out; c.ws = ws; c.st = static_cast<hipStream_t>(stream);
    c.knobs.form = tune_get("RLVI_MSTEP_FORM", -1);
    c.knobs.force_g = tune_get("RLVI_MSTEP_G", 0);
    c.knobs.cuwide = tune_get("RLVI_MSTEP_CUWIDE", 1);
    c.knobs.hold = tune_get("RLVI_MSTEP_HOLD", ws_option(ws, WSOPT_LOGITS_FROM_HBM, 0) ? -1 : 0);
    c.knobs.gen = tune_get("RLVI_MSTEP_GEN", -1);
    c.part = reinterpret_cast<double *>(base + (out == nullptr ? WS_PART_OFF : WS_PART2_OFF));
    c.status = reinterpret_cast<int32_t *>(base);
    c.accum = out == nullptr ? 1 : 0;
    c.inv_rows100 = 100.0 / (double)B;
    c.cus = device_info().cus;
    // widest vector for which every row start and the row length are aligned
    auto ok = [&](int v) { return vec_fits<T>(v, C, {{logits, ld}, {grad, ldg}}); };
    constexpr int VMAX = 16 / (int)sizeof(T);
    if constexpr (sizeof(T) == 2) {
        // bf16 / fp16 rows of an odd number of elements (single 2-byte elements in the general forms), at least
        // 32 768 of them, dense, 16-byte aligned: the word-wise wave tile.  (Every 2-byte decision here and in
        // dispatch_gk was tuned on bytes, not on the format: fp16 takes the form bf16 takes at every shape.)
        if ((C & 1) != 0 && C >= 9 && C <= 127 && B >= 16 * 2048 && ld == C && (grad == nullptr || ldg == C) &&
            ((uintptr_t)logits % 16) == 0 && ((uintptr_t)grad % 16) == 0 && c.knobs.form != 0 && c.knobs.force_g == 0)
            return launch_bf16w(c);
    }
    if constexpr (VMAX == 8) {
        if (ok(8)) return dispatch_gk<T, 8>(c);
    }
    if (ok(4)) return dispatch_gk<T, 4>(c);
    if (ok(2)) return dispatch_gk<T, 2>(c);
    return dispatch_gk<T, 1>(c);
}

}  // namespace rlvi

extern "C" int rlvi_mstep_fwd_bwd_f32(const float *logits, int64_t ld, const int64_t *labels,
                                      const int64_t *idx, const float *weights, float *residuals,
                                      int64_t N, int64_t B, int64_t C, float inv_scale,
                                      float *grad_logits, int64_t ldg, float *out, void *ws,
                                      void *stream) {
    return rlvi::mstep_entry<float>(logits, ld, labels, idx, weights, residuals, N, B, C,
                                    inv_scale, nullptr, grad_logits, ldg, out, ws, stream);
}

extern "C" int rlvi_mstep_fwd_bwd_bf16(const uint16_t *logits, int64_t ld, const int64_t *labels,
                                       const int64_t *idx, const float *weights, float *residuals,
                                       int64_t N, int64_t B, int64_t C, float inv_scale,
                                       uint16_t *grad_logits, int64_t ldg, float *out, void *ws,
                                       void *stream) {
    return rlvi::mstep_entry<uint16_t>(logits, ld, labels, idx, weights, residuals, N, B, C,
                                       inv_scale, nullptr, grad_logits, ldg, out, ws, stream);
}

extern "C" int rlvi_mstep_fwd_bwd_f16(const uint16_t *logits, int64_t ld, const int64_t *labels,
                                      const int64_t *idx, const float *weights, float *residuals,
                                      int64_t N, int64_t B, int64_t C, float inv_scale,
                                      const float *grad_scale, uint16_t *grad_logits, int64_t ldg,
                                      float *out, void *ws, void *stream) {
    return rlvi::mstep_entry<rlvi::f16_t>(reinterpret_cast<const rlvi::f16_t *>(logits), ld, labels, idx, weights,
                                          residuals, N, B, C, inv_scale, grad_scale,
                                          reinterpret_cast<rlvi::f16_t *>(grad_logits), ldg, out, ws, stream);
}

// Reduce (and clear) the partial records that accumulate-mode M-step calls left in the workspace.
extern "C" int rlvi_mstep_reduce_f32(float *out, double scale, void *ws, void *stream) {
    if (!out || !ws) return RLVI_E_NULL;
    double *part = reinterpret_cast<double *>(static_cast<char *>(ws) + rlvi::WS_PART_OFF);
    return rlvi::launch(rlvi::mstep_finalize_kernel, dim3(1), dim3(256), 0,
                        static_cast<hipStream_t>(stream), part, (int)rlvi::MSTEP_MAX_BLOCKS, scale, out, 1);
}
