// The k smallest of n fp32 values in one workgroup of SEL_BLOCK threads, no sort (select_smallest_kernel,
// jocor_select_kernel).
//
// A 4-pass radix select on the order-preserving key f32_key (8 bits per pass, LDS histogram, the bin holding the
// k-th element fixes the next byte) finds the key T of the k-th smallest value; values with key < T are kept, and of
// those with key == T the first (k - #{key < T}) in index order -- the order a stable argsort gives.  NaN orders
// last, as in numpy; -0.0 orders before +0.0.  k <= 0 keeps nothing, k >= n everything.
#pragma once
#include "rlvi_common.h"

namespace rlvi {

constexpr int SEL_BLOCK = 1024;
constexpr int SEL_NW = SEL_BLOCK / WAVE;
constexpr int SEL_U = 8;                     // loads in flight per thread in the sweeps

// The values are value(src[i]), 0 <= i < n: src[i] is read once per sweep (four histogram passes and a final sweep)
// and value is applied after the loads, so that SEL_U loads stay in flight.  emit(i, value, keep) is called once per
// i by the thread that owns i (thread i mod SEL_BLOCK, in every sweep), after its last read of src[i]: emit may
// overwrite src[i].  Call from all SEL_BLOCK threads of the workgroup.
template <class Value, class Emit>
__device__ __forceinline__ void select_smallest_block(const float *src, int64_t n, int64_t k, Value value,
                                                      Emit emit) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh_prefix, sh_need, sh_ties;
    __shared__ unsigned wcount[SEL_NW];
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    const bool none = k <= 0, all = k >= n;
    unsigned T = 0xFFFFFFFFu, need = 0u, ties = 0u;
    if (!none && !all) {
        if (tid == 0) { sh_prefix = 0u; sh_need = (unsigned)k; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const unsigned prefix = sh_prefix;
            // SEL_U independent loads in flight per thread and trip: a trip is latency-bound otherwise
            for (int64_t base = 0; base < n; base += (int64_t)SEL_U * SEL_BLOCK) {
                float v[SEL_U];
#pragma unroll
                for (int j = 0; j < SEL_U; ++j) {
                    const int64_t i = base + (int64_t)j * SEL_BLOCK + tid;
                    v[j] = i < n ? src[i] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < SEL_U; ++j) {
                    const int64_t i = base + (int64_t)j * SEL_BLOCK + tid;
                    const unsigned key = f32_key(value(v[j]));
                    // candidates: keys that agree with the prefix in the bytes fixed so far
                    const bool cand = i < n && (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
                    const unsigned bin = (key >> shift) & 255u;
                    // values cluster in a few bins of the leading bytes, where 64 lanes adding to one LDS address
                    // would serialise: one add per bin for the wave's (up to) two most common bins, plain adds
                    // for the rest
                    unsigned long long pending = __ballot(cand);
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        if (!pending) break;
                        const int leader = __ffsll((long long)pending) - 1;
                        const unsigned lb = (unsigned)__shfl((int)bin, leader);
                        const unsigned long long same = __ballot(cand && bin == lb) & pending;
                        if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
                        pending &= ~same;
                    }
                    if ((pending >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
                }
            }
            __syncthreads();
            if (wave == 0) {
                // the bin holding the need-th candidate: a prefix sum over the 256 bins, four per lane
                unsigned h[4], tot = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hist[4 * lane + j]; tot += h[j]; }
                unsigned inc = tot;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const unsigned t = (unsigned)__shfl_up((int)inc, o);
                    if (lane >= o) inc += t;
                }
                const unsigned nd = sh_need;
                unsigned pre = inc - tot;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (pre < nd && nd <= pre + h[j]) {      // exactly one bin of the wave holds it
                        sh_need = nd - pre;
                        sh_prefix = prefix | ((unsigned)(4 * lane + j) << shift);
                        sh_ties = h[j];                      // after the last pass: values with key == T
                    }
                    pre += h[j];
                }
            }
            __syncthreads();
        }
        T = sh_prefix;
        need = sh_need;
        ties = sh_ties;
    }
    if (none || all || ties == need) {
        // no ranking among equal values: a key test per element, SEL_U elements in flight per thread
        for (int64_t base = 0; base < n; base += (int64_t)SEL_U * SEL_BLOCK) {
            float v[SEL_U];
#pragma unroll
            for (int j = 0; j < SEL_U; ++j) {
                const int64_t i = base + (int64_t)j * SEL_BLOCK + tid;
                v[j] = i < n ? src[i] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < SEL_U; ++j) {
                const int64_t i = base + (int64_t)j * SEL_BLOCK + tid;
                if (i < n) {
                    const float x = value(v[j]);
                    emit(i, x, all || (!none && f32_key(x) <= T));
                }
            }
        }
        return;
    }
    // ties beyond the quota: take the first `need` of them in index order
    unsigned running = 0u;
    for (int64_t base = 0; base < n; base += SEL_BLOCK) {
        const int64_t i = base + tid;
        const float v = i < n ? value(src[i]) : 0.0f;
        const unsigned key = i < n ? f32_key(v) : 0xFFFFFFFFu;
        const bool tie = i < n && key == T;
        const unsigned long long bal = __ballot(tie);
        const unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned off = running, total = 0u;
#pragma unroll
        for (int w = 0; w < SEL_NW; ++w) {
            const unsigned c = wcount[w];
            if (w < wave) off += c;
            total += c;
        }
        const bool keep = key < T || (tie && off + before < need);
        running += total;
        __syncthreads();
        if (i < n) emit(i, v, keep);
    }
}

}  // namespace rlvi
