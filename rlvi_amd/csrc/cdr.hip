// CDR's gradient masking over all weight tensors of a network, without a sort and without a concatenated copy.
//
// Replaces deep-learning/methods/train_cdr.py:22-44: torch.cat of every covered gradient and parameter (:22-29),
// metric = |g * v| (:30), torch.topk(metric, nz) read for its last value (:33-34), and per tensor the product again,
// the compare, the cast, the scale by clip and the multiply into the gradient (:40-44).
//
// Only the nz-th largest metric and one masked multiply are needed.  |g * v| is a non-negative fp32 value, so its bit
// pattern is an order-preserving 31-bit integer key; the nz-th largest key is found by a radix descent, 11 + 10 + 10
// bits, most significant first, over a TABLE of segments {v, g, n, first chunk} (one per covered tensor) that the
// caller keeps on the device:
//
//   cdr_hist_kernel<0>   every workgroup walks its chunks (CDR_CHUNK elements of one segment each), counts bits 30..20
//                        of the keys in LDS and adds its non-empty bins to the global histogram (integer atomics: the
//                        totals do not depend on the arrival order, so every run gives the same bits);
//   cdr_hist_kernel<1>   every workgroup first scans histogram 0 from the top for the bin that holds rank nz (all
//                        workgroups find the same bin; workgroup 0 writes it down), then counts bits 19..10 of the
//                        keys inside that bin;
//   cdr_hist_kernel<2>   the same one level down: bits 9..0;
//   cdr_apply_kernel     scans histogram 2: the threshold key is now known to the bit, and so is kept = (keys above) +
//                        (keys equal) -- no atomics; then g = m * g with m = key >= threshold ? clip : 0, written as
//                        that multiplication (the signed zeros and the inf * 0 = NaN of the reference).
//
// Five launches per call (the first zeroes the 16 KiB of histograms) whatever the number of tensors; prefix and rank
// stay on the device.
// A NaN metric has the largest keys (torch.topk orders it the same way).  Same-address LDS atomics: a gradient's
// metrics sit in a few exponents, so a few dozen of the 2048 first-level bins take nearly every increment; the LDS
// histogram is kept in CDR_REPL copies, lane l adding to copy l % CDR_REPL (adjacent banks), which divides the number
// of lanes that meet on one address.
#include "rlvi_common.h"

namespace rlvi {

constexpr int CDR_BLOCK = 256;
constexpr int CDR_WGS_PER_CU = 2;            // workgroups per CU of the histogram and apply passes (profiles/r07_cdr.md)
constexpr int CDR_CHUNK = 4096;              // elements per chunk: four 16-byte pieces per lane
constexpr int CDR_REPL = 4;                  // copies of the LDS histogram
constexpr int CDR_BINS0 = 2048, CDR_BINS1 = 1024, CDR_BINS2 = 1024;
constexpr size_t CDR_HIST_WORDS = CDR_BINS0 + CDR_BINS1 + CDR_BINS2;
constexpr size_t CDR_SCRATCH_BYTES = CDR_HIST_WORDS * sizeof(uint32_t) + 256;

struct CdrSeg {                              // 32 bytes; the table is nseg of them and a closing entry
    const float *v;
    float *g;
    int64_t n;
    int64_t first_chunk;                     // closing entry: the number of chunks
};

struct CdrState {                            // where the descent stands after a level
    uint32_t prefix;                         // the key bits fixed so far (right-aligned)
    uint32_t rank;                           // the wanted key is the rank-th largest among the keys with this prefix
    unsigned long long above;                // keys larger than every key with this prefix
};

template <int LEVEL>
struct CdrLevel;
template <>
struct CdrLevel<0> { static constexpr int BINS = CDR_BINS0, SHIFT = 20, OFF = 0; };
template <>
struct CdrLevel<1> { static constexpr int BINS = CDR_BINS1, SHIFT = 10, OFF = CDR_BINS0; };
template <>
struct CdrLevel<2> { static constexpr int BINS = CDR_BINS2, SHIFT = 0, OFF = CDR_BINS0 + CDR_BINS1; };

__device__ __forceinline__ uint32_t cdr_key(float g, float v) {
    return __float_as_uint(__fmul_rn(g, v)) & 0x7FFFFFFFu;          // bits(fabsf(g * v))
}

// The segment of chunk c: first_chunk[s] <= c < first_chunk[s + 1].  `s` is where the last search ended (a workgroup's
// chunks only go up), so after the first call the walk is a step or two.
__device__ __forceinline__ int cdr_find_segment(const CdrSeg *__restrict__ table, int nseg, int64_t c, int s) {
    if (s < 0) {
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[mid].first_chunk <= c) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
    while (s + 1 < nseg && table[s + 1].first_chunk <= c) ++s;
    return s;
}

// Every element of [lo, hi) of one segment, once: 16-byte pieces of g where its address allows, the pieces of v
// likewise when v sits at the same offset from a 16-byte boundary (else four 4-byte loads), and up to three single
// elements at either end.  f(g_i, v_i) returns the new g_i; it is stored when WRITE.  The pointers come out of the
// table, so the compiler cannot know their address space: they are cast to global memory here (global_load /
// global_store instead of the flat forms).
typedef __attribute__((address_space(1))) float cdr_gf;
typedef __attribute__((address_space(1))) vf4 cdr_gf4;

template <bool WRITE, class F>
__device__ __forceinline__ void cdr_visit(const float *v_, float *g_, int64_t lo, int64_t hi, F f) {
    const cdr_gf *__restrict__ v = (const cdr_gf *)v_;
    cdr_gf *__restrict__ g = (cdr_gf *)g_;
    const int tid = threadIdx.x;
    int64_t head = (int64_t)(((16 - ((uintptr_t)(g_ + lo) & 15)) & 15) >> 2);
    if (head > hi - lo) head = hi - lo;
    const int64_t nvec = (hi - lo - head) >> 2;
    const int64_t body = lo + head;
    const int64_t tail = body + 4 * nvec;
    if (tid < head) {
        const float r = f(g[lo + tid], v[lo + tid]);
        if (WRITE) g[lo + tid] = r;
    }
    if (tid >= 64 && tid - 64 < hi - tail) {
        const int64_t i = tail + tid - 64;
        const float r = f(g[i], v[i]);
        if (WRITE) g[i] = r;
    }
    const bool v_vec = (((uintptr_t)(v_ + body)) & 15) == 0;
    constexpr int PIECES = CDR_CHUNK / (4 * CDR_BLOCK);
    vf4 gg[PIECES], vv[PIECES];
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
        const int64_t q = (int64_t)p * CDR_BLOCK + tid;
        if (q < nvec) {
            gg[p] = *(const cdr_gf4 *)(g + body + 4 * q);
            if (v_vec) {
                vv[p] = *(const cdr_gf4 *)(v + body + 4 * q);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) vv[p][e] = v[body + 4 * q + e];
            }
        }
    }
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
        const int64_t q = (int64_t)p * CDR_BLOCK + tid;
        if (q < nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) gg[p][e] = f(gg[p][e], vv[p][e]);
            if (WRITE) *(cdr_gf4 *)(g + body + 4 * q) = gg[p];
        }
    }
}

// One level of the descent, by every workgroup alike: the highest bin b with (keys in bins >= b) >= rank.  Returns the
// state one level down; *at_bin receives hist[b].
template <int BINS>
__device__ __forceinline__ CdrState cdr_descend(const uint32_t *__restrict__ hist, CdrState st, uint32_t *lds,
                                                uint32_t *at_bin) {
    constexpr int PER = BINS / CDR_BLOCK;
    const int tid = threadIdx.x;
    uint32_t h[PER], mine = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        h[j] = hist[tid * PER + j];
        mine += h[j];
    }
    // lds[t] = keys in the bins of threads t .. 255 (a suffix sum over the workgroup)
    __syncthreads();
    lds[tid] = mine;
    __syncthreads();
    for (int off = 1; off < CDR_BLOCK; off <<= 1) {
        const uint32_t add = tid + off < CDR_BLOCK ? lds[tid + off] : 0u;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[tid], excl = tid + 1 < CDR_BLOCK ? lds[tid + 1] : 0u;
    __syncthreads();
    if (incl >= st.rank && excl < st.rank) {             // exactly one thread: the suffix sums only fall
        uint32_t acc = excl;
#pragma unroll
        for (int j = PER - 1; j >= 0; --j) {
            if (acc < st.rank && acc + h[j] >= st.rank) {
                lds[0] = (uint32_t)(tid * PER + j);
                lds[1] = acc;
                lds[2] = h[j];
            }
            acc += h[j];
        }
    }
    __syncthreads();
    const uint32_t bin = lds[0], over = lds[1];
    *at_bin = lds[2];
    __syncthreads();
    CdrState nx;
    nx.prefix = st.prefix * (uint32_t)BINS + bin;
    nx.rank = st.rank - over;
    nx.above = st.above + over;
    return nx;
}

__device__ __forceinline__ uint32_t *cdr_hist(void *scratch, int off) { return static_cast<uint32_t *>(scratch) + off; }
__device__ __forceinline__ CdrState *cdr_states(void *scratch) {
    return reinterpret_cast<CdrState *>(static_cast<uint32_t *>(scratch) + CDR_HIST_WORDS);
}

// The histograms and the states start from zero in every call (a kernel, not a memset node: a captured graph that
// held the memset replayed with the counts of the call before still in place).
__global__ __launch_bounds__(CDR_BLOCK) void cdr_zero_kernel(uint32_t *__restrict__ words, int n) {
    const int i = blockIdx.x * CDR_BLOCK + threadIdx.x;
    if (i < n) words[i] = 0u;
}

template <int LEVEL>
__global__ __launch_bounds__(CDR_BLOCK) void cdr_hist_kernel(const CdrSeg *__restrict__ table, int nseg,
                                                             int64_t chunks, uint32_t nz, void *scratch) {
    using Lv = CdrLevel<LEVEL>;
    constexpr int BINS = Lv::BINS;
    __shared__ uint32_t lh[BINS * CDR_REPL];
    __shared__ uint32_t scan[CDR_BLOCK];
    const int tid = threadIdx.x;
    for (int i = tid; i < BINS * CDR_REPL; i += CDR_BLOCK) lh[i] = 0;

    CdrState st{0u, nz, 0ull};
    if constexpr (LEVEL > 0) {
        using Up = CdrLevel<LEVEL - 1>;
        uint32_t unused;
        if constexpr (LEVEL == 2) st = cdr_states(scratch)[0];
        st = cdr_descend<Up::BINS>(cdr_hist(scratch, Up::OFF), st, scan, &unused);
        if (blockIdx.x == 0 && tid == 0) cdr_states(scratch)[LEVEL - 1] = st;
    }
    __syncthreads();
    const uint32_t prefix = st.prefix;
    uint32_t *mycopy = lh + (tid & (CDR_REPL - 1));

    int s = -1;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        s = cdr_find_segment(table, nseg, c, s);
        const CdrSeg sg = table[s];
        const int64_t lo = (c - sg.first_chunk) * CDR_CHUNK;
        const int64_t hi = lo + CDR_CHUNK < sg.n ? lo + CDR_CHUNK : sg.n;
        cdr_visit<false>(sg.v, sg.g, lo, hi, [&](float g, float v) {
            const uint32_t key = cdr_key(g, v);
            if constexpr (LEVEL == 0) {
                atomicAdd(mycopy + (key >> Lv::SHIFT) * CDR_REPL, 1u);
            } else if ((key >> (Lv::SHIFT + 10)) == prefix) {
                atomicAdd(mycopy + ((key >> Lv::SHIFT) & (BINS - 1)) * CDR_REPL, 1u);
            }
            return g;
        });
    }
    __syncthreads();
    uint32_t *gh = cdr_hist(scratch, Lv::OFF);
    for (int b = tid; b < BINS; b += CDR_BLOCK) {
        uint32_t n = 0;
#pragma unroll
        for (int r = 0; r < CDR_REPL; ++r) n += lh[b * CDR_REPL + r];
        if (n) atomicAdd(gh + b, n);
    }
}

__global__ __launch_bounds__(CDR_BLOCK) void cdr_apply_kernel(const CdrSeg *__restrict__ table, int nseg,
                                                              int64_t chunks, float clip, void *scratch,
                                                              float *__restrict__ thr_out,
                                                              int64_t *__restrict__ kept_out) {
    __shared__ uint32_t scan[CDR_BLOCK];
    using Up = CdrLevel<2>;
    uint32_t equal;
    const CdrState st = cdr_descend<Up::BINS>(cdr_hist(scratch, Up::OFF), cdr_states(scratch)[1], scan, &equal);
    const uint32_t thr_key = st.prefix;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *thr_out = __uint_as_float(thr_key);
        *kept_out = (int64_t)(st.above + equal);
    }
    int s = -1;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        s = cdr_find_segment(table, nseg, c, s);
        const CdrSeg sg = table[s];
        const int64_t lo = (c - sg.first_chunk) * CDR_CHUNK;
        const int64_t hi = lo + CDR_CHUNK < sg.n ? lo + CDR_CHUNK : sg.n;
        cdr_visit<true>(sg.v, sg.g, lo, hi, [&](float g, float v) {
            const float m = cdr_key(g, v) >= thr_key ? clip : 0.0f;
            return __fmul_rn(m, g);
        });
    }
}

}  // namespace rlvi

using namespace rlvi;

extern "C" size_t rlvi_cdr_table_bytes(int nseg) {
    return nseg < 1 ? 0 : ((size_t)nseg + 1) * sizeof(CdrSeg);
}

extern "C" size_t rlvi_cdr_scratch_bytes(int nseg) {
    return nseg < 1 ? 0 : CDR_SCRATCH_BYTES;
}

extern "C" int rlvi_cdr_table_fill(void *host_buf, const void *const *v, void *const *g, const int64_t *n, int nseg,
                                   int64_t *total, int64_t *chunks) {
    if (!host_buf || !v || !g || !n || !total || !chunks) return RLVI_E_NULL;
    if (nseg < 1) return RLVI_E_SHAPE;
    if ((uintptr_t)host_buf & 7) return RLVI_E_ALIGN;
    for (int i = 0; i < nseg; ++i) {
        if (!v[i] || !g[i]) return RLVI_E_NULL;
        if (n[i] < 1) return RLVI_E_SHAPE;
        if (((uintptr_t)v[i] & 3) || ((uintptr_t)g[i] & 3)) return RLVI_E_ALIGN;
    }
    CdrSeg *t = static_cast<CdrSeg *>(host_buf);
    int64_t sum = 0, c = 0;
    for (int i = 0; i < nseg; ++i) {
        t[i].v = static_cast<const float *>(v[i]);
        t[i].g = static_cast<float *>(g[i]);
        t[i].n = n[i];
        t[i].first_chunk = c;
        sum += n[i];
        c += (n[i] + CDR_CHUNK - 1) / CDR_CHUNK;
    }
    t[nseg].v = nullptr;
    t[nseg].g = nullptr;
    t[nseg].n = 0;
    t[nseg].first_chunk = c;
    *total = sum;
    *chunks = c;
    return 0;
}

extern "C" int rlvi_cdr_mask_f32(const void *table_dev, int nseg, int64_t total, int64_t chunks, int64_t nz,
                                 float clip, void *scratch, size_t scratch_bytes, float *thr_out, int64_t *kept_out,
                                 void *stream) {
    if (!table_dev || !scratch || !thr_out || !kept_out) return RLVI_E_NULL;
    if (nseg < 1 || total < 1 || nz < 1 || nz > total) return RLVI_E_SHAPE;
    // every segment has a chunk, and none more than its elements
    if (chunks < nseg || chunks > total) return RLVI_E_SHAPE;
    if (total >= (int64_t)1 << 32) return RLVI_E_LIMIT;                     // the counts are 32-bit
    if (((uintptr_t)table_dev & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)thr_out & 3) ||
        ((uintptr_t)kept_out & 7))
        return RLVI_E_ALIGN;
    if (scratch_bytes < CDR_SCRATCH_BYTES) return RLVI_E_WS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CdrSeg *table = static_cast<const CdrSeg *>(table_dev);
    int64_t nb = (int64_t)device_info().cus * CDR_WGS_PER_CU;
    if (nb > chunks) nb = chunks;
    if (nb < 1) nb = 1;
    const dim3 grid((unsigned)nb), block(CDR_BLOCK);
    constexpr int words = (int)(CDR_SCRATCH_BYTES / sizeof(uint32_t));
    int rc = launch(cdr_zero_kernel, dim3((words + CDR_BLOCK - 1) / CDR_BLOCK), block, 0, st,
                    static_cast<uint32_t *>(scratch), words);
    if (rc != 0) return rc;
    const uint32_t rank = (uint32_t)nz;
    rc = launch(cdr_hist_kernel<0>, grid, block, 0, st, table, nseg, chunks, rank, scratch);
    if (rc != 0) return rc;
    rc = launch(cdr_hist_kernel<1>, grid, block, 0, st, table, nseg, chunks, rank, scratch);
    if (rc != 0) return rc;
    rc = launch(cdr_hist_kernel<2>, grid, block, 0, st, table, nseg, chunks, rank, scratch);
    if (rc != 0) return rc;
    return launch(cdr_apply_kernel, grid, block, 0, st, table, nseg, chunks, clip, scratch, thr_out, kept_out);
}
