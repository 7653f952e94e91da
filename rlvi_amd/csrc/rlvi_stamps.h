// Lab stamps of the cooperating kernels: the one slot table and the helpers that write it.
//
// A -DRLVI_STAMPS=1 build (tools/build_variants.py stamps=-DRLVI_STAMPS=1; load it with RLVI_LIB_PATH) run with
// RLVI_TJ_DEBUG (E-step solve, in-batch E+M) or RLVI_THR_DEBUG (threshold) leaves 100 MHz wall-clock stamps and value
// dumps in 8-byte slots at the start of the workspace's scratch region (stamp_base(), rlvi_common.h; from Python
// ops.debug_scratch_offset()).  In the product build all of it is compiled out: the stamp pointer, its counter and
// the guards around every dump cost the trajectory kernels some twenty registers, i.e. a wave per SIMD.
//
// This header is the only place that knows a slot number.  Kernels name a region (ST_<name>) and an index inside it;
// tools/stamps.py parses the list below, so the readers have no table of their own.
//
// What else lives in the scratch (ws_bytes_for reserves the table's extent there in a stamps build):
//   * the scratch is sized for the `l` and `e` rows of an in-batch E+M (8 bytes per sample from the region's first
//     byte).  The one-launch kernels of fused_em.hip keep those rows in registers; a form that puts them back there
//     must not run stamped, or must read its rows before workgroup 0 stamps over the first 1000 samples' worth;
//   * aux.hip's rlvi_linreg_losses_f64 keeps its per-workgroup partials there (up to 256 doubles: slots 0..255)
//     between its two launches.  It takes no stamps, but a call of it wipes the E-step's and the threshold's stamps
//     in those slots -- read the stamps before the next residual call (tools/lab/linreg_phases.py, whose standard.hip
//     scheme dumps its own buffer at slot 0, and the M-step's -DRLVI_MSTEP_STAMPS dump overwrite the table likewise:
//     one scheme per run);
//   * stamps and dumps do not disturb any result: no kernel reads the table.  Slots of an earlier launch stay until
//     overwritten, so readers test a slot for 0 only on a workspace they created or cleared themselves;
//   * the E-step and the threshold share the table but no region: the stamps of one survive a launch of the other.
#pragma once
#include <hip/hip_runtime.h>

#ifndef RLVI_STAMPS
#define RLVI_STAMPS 0
#endif

// X(name, first slot, slots, "what it holds and who writes it")
#define RLVI_STAMP_TABLE(X)                                                                                            \
    X(THR_SEQ, 32, 60, "threshold_radix_kernel, workgroup 0 thread 0: sequential wall-clock stamps of its phases")     \
    X(THR_COUNT, 95, 1, "threshold_radix_kernel: how many of THR_SEQ were taken")                                      \
    X(TJ_FINITE, 102, 1, "tj_chain, first round: ballot of the lanes whose totals are finite")                         \
    X(TJ_SCALE, 103, 1, "tj_chain, first round: exp(shift - min) as fp32 bits")                                        \
    X(TJ_TOTALS, 104, 24, "tj_chain, first round: {S, P, Q} of nodes 0..7 as fp64 bits")                               \
    X(TJ_ROUND_OK, 128, 1, "tj_chain, first round: whether the round's totals were usable")                            \
    X(TJ_IT_DELTA, 129, 1, "tj_chain, first round: pair (it, delta as fp32 bits)")                                     \
    X(TJ_NODES, 130, 64, "tj_chain, first round, per lane: pair (guessed node rn, corrected node rnew)")                \
    X(SOLVE_SEQ, 200, 60, "trajb_solve, workgroup 0 thread 0: sequential wall-clock stamps of its phases")             \
    X(SOLVE_COUNT, 260, 1, "trajb_solve: how many of SOLVE_SEQ were taken")                                            \
    X(SOLVE_ROUNDS, 264, 24, "trajb_solve, per round: pair ((Ke << 8) | it, delta as fp32 bits)")                      \
    X(TJ_ROUND_NODES, 400, 256, "tj_chain, rounds 0..3 x 64 lanes: pair (rn, rnew)")                                   \
    X(TJ_ACCEPT, 699, 1, "tj_chain acceptance test: pair (accepted without verification, it)")                         \
    X(TJ_ERR_BAND, 700, 64, "tj_chain acceptance test, per lane: pair (estimated step error, band)")                    \
    X(TJ_EK_SLOPE, 764, 64, "tj_chain acceptance test, per lane: pair (E_k, slope)")                                   \
    X(TJ_SK_RHO, 828, 64, "tj_chain acceptance test, per lane: pair (s_k, rho_k) in front of the scan")                \
    X(SOLVE_WMIN, 898, 1, "trajb_solve, sample-split stage A of workgroup 0: the minimum it published, fp32 bits")     \
    X(SOLVE_TOTALS_MIN, 900, 64, "trajb_solve, first round, per lane: pair (granules nq, total's minimum val[4])")     \
    X(KERNEL_CYCLES, 966, 1, "estep_trajb_kernel: shader-clock cycles from entry to the end of the solve")             \
    X(KERNEL_TICKS, 967, 1, "estep_trajb_kernel: wall-clock ticks over the same stretch")                              \
    X(FUSED_SEQ, 970, 8, "fused_em kernel: wall clock at {start, loads issued, rows, barrier, solved, grad, -, out}")  \
    X(SUMS_ARITH, 980, 1, "trajb_solve node-split sums, first round: wall clock behind the arithmetic")                \
    X(SUMS_BFLY, 981, 1, "trajb_solve node-split sums, first round: wall clock behind the butterflies")                \
    X(RED_BARRIER, 982, 1, "trajb_solve reducer, first round: wall clock behind its barrier")                          \
    X(STAGED_CYCLES, 983, 1, "trajb_solve: shader clock when the slice is staged")                                     \
    X(SUMS_CYCLES, 984, 1, "trajb_solve node-split sums, first round: shader clock behind the arithmetic")             \
    X(STAGED_CLOCK, 985, 1, "trajb_solve: wall clock when the slice is staged")                                        \
    X(ENTRY, 986, 3, "estep_trajb_kernel: wall clock at {first instruction, first data loads issued, slice landed}")   \
    X(RED_PUBLISH, 989, 1, "trajb_solve reducer, first round: wall clock with the granule to publish in hand")         \
    X(CHAIN_SEQ, 990, 6, "tj_chain, first round: wall clock at {entry, prepared, chain, trust/tail, acceptance, out}") \
    X(HELPER, 996, 2, "tj_accept_guess (the helper wave), first round: wall clock at {start, done}")                   \
    X(CHAIN_BARRIER2, 998, 1, "tj_chain, first round: wall clock past its second workgroup barrier")

namespace rlvi {

enum StampSlot {
#define RLVI_X(name, first, count, what) ST_##name,
    RLVI_STAMP_TABLE(RLVI_X)
#undef RLVI_X
    ST_REGIONS
};

struct StampRegion {
    int first, count;
};
constexpr StampRegion STAMP_REGIONS[ST_REGIONS] = {
#define RLVI_X(name, first, count, what) {first, count},
    RLVI_STAMP_TABLE(RLVI_X)
#undef RLVI_X
};
constexpr int stamp_first(StampSlot s) { return STAMP_REGIONS[s].first; }
constexpr int stamp_count(StampSlot s) { return STAMP_REGIONS[s].count; }
constexpr int STAMP_EXTENT = 1000;                      // slots of the table
constexpr unsigned long STAMP_BYTES = 8ul * STAMP_EXTENT;   // what a stamps build needs of the scratch

constexpr bool stamp_table_sound() {
    for (int a = 0; a < ST_REGIONS; ++a) {
        const StampRegion &r = STAMP_REGIONS[a];
        if (r.first < 0 || r.count < 1 || r.first + r.count > STAMP_EXTENT) return false;
        for (int b = 0; b < a; ++b) {
            const StampRegion &o = STAMP_REGIONS[b];
            if (r.first < o.first + o.count && o.first < r.first + r.count) return false;
        }
    }
    return true;
}
static_assert(stamp_table_sound(), "stamp regions must not overlap and must lie inside STAMP_EXTENT");

// The address of a region for a kernel that is handed one, and back to the table's base inside that kernel.
// (The threshold's launcher passes its region and not the base: that is the byte offset the product build always
//  passed, so its host code stays what it was.)
template <StampSlot S>
inline unsigned long long *stamp_region(unsigned long long *base) {
    return base + stamp_first(S);
}
template <StampSlot S>
__device__ __forceinline__ unsigned long long *stamp_table_of(unsigned long long *region) {
    return region != nullptr ? region - stamp_first(S) : nullptr;
}

// ---- the writers.  dbg: the table's base, or nullptr (no debug knob set: nothing is written); who: which thread(s)
// of which workgroup and round write; S, i: slot i of region S.  All of them fold to nothing in the product build.
// Every `who` begins with `RLVI_STAMPS &&` (directly or through a named predicate of its function): an argument is
// evaluated at the call, and a dead read of the workgroup id or a dead short-circuit branch is enough to move the
// product kernels' register allocation (measured on estep_trajb_kernel; tools/isa_same.py shows it).
#define RLVI_STAMP_ON(S, i) (RLVI_STAMPS && dbg != nullptr && who && (i) >= 0 && (i) < stamp_count(S))

// the 100 MHz wall clock
template <StampSlot S>
__device__ __forceinline__ void stamp_clock(unsigned long long *dbg, bool who, int i = 0) {
    if (RLVI_STAMP_ON(S, i)) dbg[stamp_first(S) + i] = wall_clock64();
}
// the shader clock (its ratio to the wall clock over a stretch is the clock the kernel ran at)
template <StampSlot S>
__device__ __forceinline__ void stamp_cycles(unsigned long long *dbg, bool who, int i = 0) {
    if (RLVI_STAMP_ON(S, i)) dbg[stamp_first(S) + i] = __builtin_amdgcn_s_memtime();
}
// a value, or a pair of 32-bit words (hi, lo) -- fp32 values go in as their bits
template <StampSlot S>
__device__ __forceinline__ void stamp_put(unsigned long long *dbg, bool who, int i, unsigned long long v) {
    if (RLVI_STAMP_ON(S, i)) dbg[stamp_first(S) + i] = v;
}
template <StampSlot S>
__device__ __forceinline__ void stamp_put(unsigned long long *dbg, bool who, int i, unsigned int hi, unsigned int lo) {
    stamp_put<S>(dbg, who, i, ((unsigned long long)hi << 32) | lo);
}
template <StampSlot S>
__device__ __forceinline__ void stamp_put(unsigned long long *dbg, bool who, int i, float hi, float lo) {
    stamp_put<S>(dbg, who, i, __float_as_uint(hi), __float_as_uint(lo));
}
// the next sequential stamp of region S; n counts them (the caller stores it with stamp_put when it is done)
template <StampSlot S>
__device__ __forceinline__ void stamp_next(unsigned long long *dbg, bool who, int &n) {
    if (RLVI_STAMP_ON(S, n)) dbg[stamp_first(S) + n++] = wall_clock64();
}
// ... staged: taken into `stage` (LDS, stamp_count(S) words) by a kernel that cannot afford a global store where it
// stamps; it copies them out with stamp_put at its end.  (An overload, not a pointer chosen at run time: that would
// be a flat store.)
template <StampSlot S>
__device__ __forceinline__ void stamp_next(unsigned long long *dbg, bool who, int &n, unsigned long long *stage) {
    if (RLVI_STAMP_ON(S, n)) stage[n++] = wall_clock64();
}
#undef RLVI_STAMP_ON

}  // namespace rlvi
