// The host side of the one-workgroup fp64 estimators' extern "C" entries (standard.hip, logreg.hip, robust_logreg.hip,
// moments.hip, robust_linreg.hip, online_sgd.hip), ONE copy of each piece.  Host code only: nothing here reaches a
// code object, the kernels and what they call live in rlvi_sl.h and the headers on it.
//   * the checks of a call in the ONE order every entry keeps, NULL -> SHAPE -> LIMIT -> ALIGN (sl_check_args; its two
//     halves sl_check_values and sl_misaligned for the entry that has checks of its own between them);
//   * the launch of SL_THREADS-wide workgroups (sl_launch: with the request for more than 64 KiB of dynamic LDS that
//     allow_dyn_lds keeps once per kernel address and device; sl_launch_plain: without, for the kernels that need none);
//   * the workspace's status word (sl_status; the lab stamps' base is stamp_base of rlvi_common.h);
//   * the dispatch tables: which instantiation takes (n, d).  Each is a function that calls its callable with a tag
//     (SlForm) carrying the template arguments -- `[&](auto f) { using F = decltype(f); return sl_launch(kernel<F::E,
//     F::DS>, ...); }` -- and, where the kernel's LDS depends on the form, the shape that goes with it:
//       sl_per_thread<1, 4, 16> (sl_samples_per_thread)   samples per thread
//       sl_linreg_form, sl_linreg_shape                   the linear regressions (standard.hip, robust_linreg.hip)
//       sl_logreg_form, sl_pad64                          the logistic regressions (logreg.hip, robust_logreg.hip)
//       sl_moments_form                                   mean, PCA and covariance, RLVI's and RRM's (moments.hip)
// A single entry is its batch entry with batch = 1: each family has ONE `template <bool BATCH>` entry function in its
// .hip file, which passes BATCH on to the kernel (the kernels' template flag: profiles/r18_batch.md).  BATCH is chosen
// outside the table's callable, not by a run-time switch inside it: a code object lists its kernels in the order the
// source first names them, and this way the order stays all single forms, then all batch forms.
#pragma once
#include <initializer_list>

#include "rlvi_sl.h"

namespace rlvi {

// ---- the checks (a null pointer counts as aligned: an optional argument passes)
inline bool sl_any_null(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (!p) return true;
    return false;
}
// in a list of required pointers: p is required only when `needed`
inline const void *sl_when(bool needed, const void *p) {
    static const char present = 0;
    return needed ? p : &present;
}
// the fp64 arrays on 8 bytes, the int32 arrays (info) on 4, the workspace on 256
inline bool sl_misaligned(std::initializer_list<const void *> f64, std::initializer_list<const void *> i32 = {},
                          const void *ws = nullptr) {
    for (const void *p : f64)
        if ((uintptr_t)p & 7) return true;
    for (const void *p : i32)
        if ((uintptr_t)p & 3) return true;
    return ((uintptr_t)ws & 255) != 0;
}
// NULL -> SHAPE -> LIMIT.  params_ok: what the entry asks of its other arguments (counts >= 0, C > 0, eps in range);
// within_limits: n, d and the entry's other sizes are what its kernels take (the batch count's limit is here).
inline int sl_check_values(std::initializer_list<const void *> required, int64_t batch, int64_t n, int64_t d,
                           bool params_ok, bool within_limits) {
    if (sl_any_null(required)) return RLVI_E_NULL;
    if (batch <= 0 || n <= 0 || d <= 0 || !params_ok) return RLVI_E_SHAPE;
    if (batch > SL_MAXBATCH || !within_limits) return RLVI_E_LIMIT;
    return 0;
}
inline int sl_check_args(std::initializer_list<const void *> required, int64_t batch, int64_t n, int64_t d,
                         bool params_ok, bool within_limits, std::initializer_list<const void *> f64,
                         std::initializer_list<const void *> i32 = {}, const void *ws = nullptr) {
    if (const int e = sl_check_values(required, batch, n, d, params_ok, within_limits)) return e;
    return sl_misaligned(f64, i32, ws) ? RLVI_E_ALIGN : 0;
}

inline int32_t *sl_status(void *ws) { return &static_cast<WsHeader *>(ws)->status; }

// ---- the launch: `grid` workgroups of SL_THREADS
template <class K, class... Args>
inline int sl_launch_plain(K kern, int64_t grid, size_t lds, hipStream_t st, Args... args) {
    return launch(kern, dim3((unsigned)grid), dim3(SL_THREADS), lds, st, args...);
}
template <class K, class... Args>
inline int sl_launch(K kern, int64_t grid, size_t lds, hipStream_t st, Args... args) {
    if (const int e = allow_dyn_lds(kern, 150 * 1024)) return e;
    return sl_launch_plain(kern, grid, lds, st, args...);
}

// ---- the dispatch tables
// E samples per thread; DS: the system (moments: the d x d algebra) padded to DS rows; NB 16-column blocks of the design;
// RES: the design resident on the chip
template <int E_, int DS_ = 0, int NB_ = 1, bool RES_ = false>
struct SlForm {
    static constexpr int E = E_, DS = DS_, NB = NB_;
    static constexpr bool RES = RES_;
};
constexpr int sl_pad64(int64_t n) { return (int)((n + 63) / 64) * 64; }

// the first E of the list whose E * SL_THREADS samples hold n; the last one beyond
template <int E0, int... ES, class F>
inline int sl_per_thread(int64_t n, F &&f) {
    if constexpr (sizeof...(ES) == 0) {
        return f(SlForm<E0>{});
    } else {
        return n <= E0 * SL_THREADS ? f(SlForm<E0>{}) : sl_per_thread<ES...>(n, f);
    }
}
template <class F>
inline int sl_samples_per_thread(int64_t n, F &&f) {
    return sl_per_thread<1, 4, 16>(n, f);
}

// Linear regression: four samples per thread up to n = 1024, sixteen beyond; the system solved padded to 12 / 16 / 20 /
// 24 / 32 rows; one or two 16-column blocks of [X | y] (column d, y, needs the second from d = 16); the design resident
// on the chip -- registers + LDS -- when n <= 1024 and d <= 23.
inline bool sl_linreg_resident(int64_t n, int64_t d) { return n <= 4 * SL_THREADS && d <= 23; }
template <class F>
inline int sl_linreg_form(int64_t n, int64_t d, F &&f) {
    if (sl_linreg_resident(n, d)) {
        if (d <= 12) return f(SlForm<4, 12, 1, true>{});
        if (d <= 15) return f(SlForm<4, 16, 1, true>{});
        if (d <= 20) return f(SlForm<4, 20, 2, true>{});
        return f(SlForm<4, 24, 2, true>{});
    }
    if (n <= 4 * SL_THREADS) return f(SlForm<4, 32, 2, false>{});      // d = 24 .. 31
    if (d <= 12) return f(SlForm<16, 12, 1, false>{});
    if (d <= 15) return f(SlForm<16, 16, 1, false>{});
    if (d <= 20) return f(SlForm<16, 20, 2, false>{});
    if (d <= 24) return f(SlForm<16, 24, 2, false>{});
    return f(SlForm<16, 32, 2, false>{});
}
// the LDS of SlShared (rlvi_linreg.h) in doubles: wsh, rsh, the solve's block, x1s where the resident design has a
// second block
constexpr size_t sl_lds_doubles(int npad, bool x1s) {
    return 2 * (size_t)npad + SL_SOLVE_DOUBLES + (x1s ? 1024 * 8 : 0);
}
struct SlLinregShape {
    int npad;           // the per-sample LDS vectors' length
    size_t lds;         // bytes, `extra_doubles` of the caller's behind SlShared's
};
inline SlLinregShape sl_linreg_shape(int64_t n, int64_t d, int extra_doubles) {
    const bool res = sl_linreg_resident(n, d);
    const int npad = res ? 1024 : sl_pad64(n);
    return {npad, (sl_lds_doubles(npad, res && d >= 16) + extra_doubles) * sizeof(double)};
}

// Logistic regression: the system of d + 1 unknowns solved padded to 4 / 16 / 24 / 32 rows; [X | 1] and the gradient's
// column in one 16-column block (d <= 14) or two.  The per-sample LDS vectors are sl_pad64(n) long.
template <class F>
inline int sl_logreg_form(int64_t n, int64_t d, F &&f) {
    return sl_samples_per_thread(n, [&](auto e) {
        constexpr int E = decltype(e)::E;
        if (d <= 3) return f(SlForm<E, 4, 1>{});
        if (d <= 14) return f(SlForm<E, 16, 1>{});
        if (d <= 23) return f(SlForm<E, 24, 2>{});
        return f(SlForm<E, 32, 2>{});
    });
}

// Mean, PCA, covariance: the d x d algebra padded to 2 / 4 / 8
template <class F>
inline int sl_moments_form(int64_t n, int64_t d, F &&f) {
    return sl_samples_per_thread(n, [&](auto e) {
        constexpr int E = decltype(e)::E;
        if (d <= 2) return f(SlForm<E, 2>{});
        if (d <= 4) return f(SlForm<E, 4>{});
        return f(SlForm<E, 8>{});
    });
}

}  // namespace rlvi
