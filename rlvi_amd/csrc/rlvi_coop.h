// The exchange between cooperating workgroups inside one launch, and on top of it the cooperative
// all-reduce of two doubles (Coop).
//
// The E-step fixed point is a serial chain of population-wide reductions.  Kernel boundaries
// cost ~1.5-1.9 us each and a software grid barrier ~4 us (MI355X_MICROARCH.md price list), so
// the chain runs inside ONE launch of G <= 256 co-resident workgroups (one per CU) that keep
// their slice of the vector in registers and exchange small records per step.  The protocol, for every
// kernel that waits on other workgroups (estep_kernel through Coop, rlvi_trajb.h, fused_em.hip's batch
// scalars, threshold.hip), is written here once:
//
//   * a record is made of self-tagged 8-byte granules {tag:32, payload:32} (`granule`, `granule_has`,
//     `granule_payload`; two of them in 16 bytes: `granule_pair`).  The data IS the flag: no fence, no
//     separate flag, and it does not matter that a 16-byte access is only granule-atomic;
//   * granules are published with relaxed atomic stores, agent scope inside a GPU and system scope into a
//     peer's inbox (`publish`), or 16 bytes at a time with a write-through `sc1` store (`rec_store16`);
//   * a reader polls with `sc1` 16-byte loads (`rec_load<N>`: N consecutive ones and one wait;
//     `rec_load_scattered`: four addresses) and uses a record only once the granules it needs carry the
//     current tag (`rec_tagged<NQ>`);
//   * every poll loop is `bounded_wait`: bounded by the wall clock (`spin_bound`), and whoever sees the
//     bound pass raises RLVI_ST_TIMEOUT and stops exchanging (the two record waits of rlvi_trajb.h's round
//     spell the same loop out: profiles/r14_exchange_layer.md);
//   * slots are double-buffered by step parity: a workgroup can publish step p+2 only after it
//     gathered step p+1, i.e. after every workgroup has finished reading step p.  Tags are base+step
//     with the base kept in the workspace (`first_tag` at entry, `close_tags` by one thread at the end),
//     so no per-launch memset is needed and graph replay is safe.
//
// What is combined is the exchange's own business: the polled values are combined in a fixed order
// (ascending workgroup per lane, then a butterfly), so every workgroup computes bit-identical totals and
// takes identical branches -- the stop decision of the fixed point can never diverge between workgroups.
#pragma once
#include "rlvi_common.h"

namespace rlvi {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

// ---- granules
__device__ __forceinline__ unsigned long long granule(uint32_t tag, uint32_t payload) {
    return ((unsigned long long)tag << 32) | payload;
}
__device__ __forceinline__ bool granule_has(unsigned long long g, uint32_t tag) { return (uint32_t)(g >> 32) == tag; }
__device__ __forceinline__ uint32_t granule_payload(unsigned long long g) { return (uint32_t)g; }
__device__ __forceinline__ vu4 granule_pair(uint32_t tag, uint32_t lo, uint32_t hi) { return (vu4){lo, tag, hi, tag}; }
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT>
__device__ __forceinline__ void publish(gu64 *p, uint32_t tag, uint32_t payload) {
    __hip_atomic_store(p, granule(tag, payload), __ATOMIC_RELAXED, SCOPE);
}

// ---- records: N consecutive 16-byte pieces at p, all in flight together
template <int N>
__device__ __forceinline__ void rec_load(const gu64 *p, vu4 *q) {
    static_assert(N >= 2 && N <= 4, "records of 32, 48 or 64 bytes");
    const unsigned long long a = (unsigned long long)(uintptr_t)p;
    if constexpr (N == 2)
        asm volatile(
            "global_load_dwordx4 %0, %2, off sc1\n\t"
            "global_load_dwordx4 %1, %2, off offset:16 sc1\n\t"
            "s_waitcnt vmcnt(0)"
            : "=&v"(q[0]), "=&v"(q[1])
            : "v"(a)
            : "memory");
    else if constexpr (N == 3)
        asm volatile(
            "global_load_dwordx4 %0, %3, off sc1\n\t"
            "global_load_dwordx4 %1, %3, off offset:16 sc1\n\t"
            "global_load_dwordx4 %2, %3, off offset:32 sc1\n\t"
            "s_waitcnt vmcnt(0)"
            : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2])
            : "v"(a)
            : "memory");
    else
        asm volatile(
            "global_load_dwordx4 %0, %4, off sc1\n\t"
            "global_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
            "global_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
            "global_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
            "s_waitcnt vmcnt(0)"
            : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3])
            : "v"(a)
            : "memory");
}
// four 16-byte pieces at four addresses
__device__ __forceinline__ void rec_load_scattered(const unsigned long long (&addr)[4], vu4 (&q)[4]) {
    asm volatile(
        "global_load_dwordx4 %0, %4, off sc1\n\t"
        "global_load_dwordx4 %1, %5, off sc1\n\t"
        "global_load_dwordx4 %2, %6, off sc1\n\t"
        "global_load_dwordx4 %3, %7, off sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3])
        : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3])
        : "memory");
}
// whether the first NQ granules of the pieces q[0 .. (NQ + 1) / 2) carry `tag`
template <int NQ>
__device__ __forceinline__ bool rec_tagged(const vu4 *q, uint32_t tag) {
    bool ok = true;
#pragma unroll
    for (int g = 0; g < NQ; ++g) ok = ok && ((g & 1) ? q[g >> 1].w : q[g >> 1].y) == tag;
    return ok;
}
// one 16-byte piece, write-through
__device__ __forceinline__ void rec_store16(gu64 *p, vu4 q) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1"
                 :
                 : "v"((unsigned long long)(uintptr_t)p), "v"(q)
                 : "memory");
}

struct OpSum {
    static __device__ __forceinline__ double ident() { return 0.0; }
    static __device__ __forceinline__ double apply(double a, double b) { return a + b; }
};
struct OpMin {
    static __device__ __forceinline__ double ident() { return __builtin_inf(); }
    static __device__ __forceinline__ double apply(double a, double b) { return b < a ? b : a; }
};
struct OpMax {
    static __device__ __forceinline__ double ident() { return -__builtin_inf(); }
    static __device__ __forceinline__ double apply(double a, double b) { return b > a ? b : a; }
};

template <class Op>
struct OpFn {
    __device__ __forceinline__ double operator()(double a, double b) const { return Op::apply(a, b); }
};
template <class Op>
struct OpFnF {
    __device__ __forceinline__ float operator()(float a, float b) const {
        return (float)Op::apply((double)a, (double)b);
    }
};
template <>
struct OpFnF<OpSum> {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
    return group_allreduce<WAVE>(v, OpFn<Op>());
}

// Default bound of an inter-workgroup wait: 100 ms of the 100 MHz wall clock (an exchange takes
// ~1 us; the bound only ends a launch whose workgroups cannot all be resident, e.g. beside another
// process's kernels).  rlvi_workspace_init writes RLVI_SPIN_BOUND_MS into the workspace header.
// (peers -- sharded over several GPUs: a peer may legitimately be late -- another process, another stream --,
//  and every wait downstream of the cross-rank hop inherits its lateness: 100 x the bound)
constexpr unsigned long long SPIN_BOUND_DEFAULT_TICKS = 10000000ull;
__device__ __forceinline__ unsigned long long spin_bound(const WsHeader *hdr, bool peers = false) {
    const unsigned long long t = hdr->spin_ticks;
    return (t != 0ull ? t : SPIN_BOUND_DEFAULT_TICKS) * (peers ? 100ull : 1ull);
}
// Polls until poll() says "done"; false if `bound` ticks passed since t0 first.  The exit condition is the
// caller's: wave-uniform (__all), per thread, or a ballot over the lanes that are there.
template <class Poll>
__device__ __forceinline__ bool bounded_wait(unsigned long long t0, unsigned long long bound, Poll poll) {
    for (unsigned spin = 0;; ++spin) {
        if (poll()) return true;
        // the wall clock is read only every 64 polls: keep the poll loop tight
        if ((spin & 63u) == 63u && wall_clock64() - t0 > bound) return false;
    }
}

// ---- a launch's tags.  first_tag: every workgroup reads the base before any workgroup can finish
// (finishing needs everybody's first publish), so the writer at the end never races this read.
// close_tags: ONE thread, at the end, with the tag of the exchange that would come next; leaves the base for
// the next launch (one tag is left free: fused_em.hip's batch scalars use it).
__device__ __forceinline__ uint32_t first_tag(WsHeader *hdr) {
    return __hip_atomic_load((gu32 *)&hdr->epoch_base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
}
__device__ __forceinline__ void close_tags(WsHeader *hdr, uint32_t next_tag) {
    __hip_atomic_store((gu32 *)&hdr->epoch_base, next_tag + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int BLOCK>
struct Coop {
    gu64 *slots;        // [2][XCHG_REPLICAS][MAX_COOP_WG][XCHG_GRANULES]
    int32_t *status;
    uint32_t tag;       // tag of the NEXT exchange
    int step;           // exchanges done so far
    int nwg;
    unsigned long long bound;   // spin bound, wall-clock ticks
    bool dead;          // a wait timed out: stop exchanging, results are invalid

    static constexpr int NW = BLOCK / WAVE;

    // nwg_ = number of exchanging workgroups (blocks 0..nwg_-1 of the grid)
    __device__ __forceinline__ void init(void *ws, int nwg_) {
        char *base = static_cast<char *>(ws);
        WsHeader *hdr = reinterpret_cast<WsHeader *>(base);
        slots = (gu64 *)(reinterpret_cast<unsigned long long *>(base + WS_XCHG_OFF));
        status = &hdr->status;
        tag = first_tag(hdr);
        step = 0;
        nwg = nwg_;
        bound = spin_bound(hdr);
        dead = false;
    }

    // Leaves base + steps in the workspace for the next launch (call from ONE thread, at the end).
    __device__ __forceinline__ void finish(void *ws) {
        close_tags(reinterpret_cast<WsHeader *>(ws), tag);
    }

    // All threads call with their per-thread partials; all threads return the global result.
    // F32WAVE: the per-thread partials are fp32 values; reduce them inside the wave in fp32 (one
    // fused v_add_f32_dpp per butterfly step instead of two DPP moves + an fp64 add), fp64 from
    // the wave partials on.
    template <class OpA, class OpB, bool F32WAVE = false>
    __device__ __forceinline__ void allreduce2(double &a, double &b) {
        constexpr int NPW = MAX_COOP_WG / WAVE;      // polling waves: one record per lane
        static_assert(NW >= NPW, "the gather needs four waves");
        __shared__ double part[2 * NW];
        __shared__ double part2[2 * NPW];
        __shared__ double bc[2];
        __shared__ int sh_dead;
        const int lane = threadIdx.x & (WAVE - 1);
        const int wave = threadIdx.x / WAVE;
        if (F32WAVE) {
            a = (double)group_allreduce<WAVE>((float)a, OpFnF<OpA>());
            b = (double)group_allreduce<WAVE>((float)b, OpFnF<OpB>());
        } else {
            a = wave_reduce<OpA>(a);
            b = wave_reduce<OpB>(b);
        }
        if (lane == 0) { part[2 * wave] = a; part[2 * wave + 1] = b; }
        if (threadIdx.x == 0) sh_dead = dead ? 1 : 0;
        __syncthreads();
        const bool xchg = nwg > 1 && !dead;          // uniform over the workgroup
        gu64 *buf = slots + (size_t)(step & 1) * XCHG_REPLICAS * MAX_COOP_WG * XCHG_GRANULES;
        if (wave == 0) {
            double ta = lane < NW ? part[2 * lane] : OpA::ident();
            double tb = lane < NW ? part[2 * lane + 1] : OpB::ident();
            ta = wave_reduce<OpA>(ta);
            tb = wave_reduce<OpB>(tb);
            if (xchg) {
                // publish: lane l stores granule l & 3 (32 contiguous bytes) of replica l >> 2
                if (lane < XCHG_GRANULES * XCHG_REPLICAS) {
                    const int gq = lane & (XCHG_GRANULES - 1), rep = lane / XCHG_GRANULES;
                    const unsigned long long bits =
                        (unsigned long long)__double_as_longlong(gq < 2 ? ta : tb);
                    const uint32_t half = (gq & 1) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
                    publish(buf + ((size_t)rep * MAX_COOP_WG + blockIdx.x) * XCHG_GRANULES + gq, tag, half);
                }
            } else if (lane == 0) {
                bc[0] = ta;
                bc[1] = tb;
            }
        }
        if (xchg) {
            // gather: waves 0..3, lane l of wave v owns workgroup 64 v + l (all records in flight
            // together); wave totals, then the four of them in a fixed order
            if (wave < NPW) {
                const int w = wave * WAVE + lane;
                const bool mine = w < nwg;
                gu64 *p = buf + ((size_t)(blockIdx.x & (XCHG_REPLICAS - 1)) * MAX_COOP_WG + (mine ? w : 0)) *
                                XCHG_GRANULES;
                // the 32-byte record: the two doubles, split in halves
                vu4 q[2] = {};
                const bool timeout = !bounded_wait(wall_clock64(), bound, [&] {
                    bool ok = true;
                    if (mine) {
                        rec_load<2>(p, q);
                        ok = rec_tagged<4>(q, tag);
                    }
                    return __all(ok) != 0;
                });
                double ga = OpA::ident(), gb = OpB::ident();
                if (mine && !timeout) {
                    ga = __longlong_as_double((long long)(((unsigned long long)q[0].z << 32) | q[0].x));
                    gb = __longlong_as_double((long long)(((unsigned long long)q[1].z << 32) | q[1].x));
                }
                ga = wave_reduce<OpA>(ga);
                gb = wave_reduce<OpB>(gb);
                if (lane == 0) {
                    part2[2 * wave] = ga;
                    part2[2 * wave + 1] = gb;
                    if (timeout) {
                        sh_dead = 1;
                        atomicOr(status, RLVI_ST_TIMEOUT);
                    }
                }
            }
            __syncthreads();
            a = part2[0];
            b = part2[1];
#pragma unroll
            for (int v = 1; v < NPW; ++v) {
                a = OpA::apply(a, part2[2 * v]);
                b = OpB::apply(b, part2[2 * v + 1]);
            }
        } else {
            __syncthreads();
            a = bc[0];
            b = bc[1];
        }
        dead = sh_dead != 0;
        ++step;
        ++tag;
    }
};

}  // namespace rlvi
