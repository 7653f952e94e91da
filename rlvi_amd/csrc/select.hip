// Small-loss selection: the k smallest of n per-sample losses as a 0/1 weight vector.
//
// Replaces the host-side  ind_sorted = np.argsort(loss.cpu()); ind_update = ind_sorted[:k]  of the
// small-loss baselines (train_usdnl.py:18-24, train_coteaching.py:18-30): the selected rows then
// get weight 1 in the streaming M-step kernel (mstep.hip) instead of being gathered into a new
// batch, so the loss/gradient pass is the same kernel the RLVI path uses.
//
// One workgroup, no sort: the radix select of rlvi_select.h (equal losses in index order -- the order a stable
// argsort gives; numpy's default sort is not stable, so which of several EQUAL losses it keeps is an implementation
// detail of the reference -- and NaN last, as in numpy).
#include "rlvi_select.h"

namespace rlvi {

__global__ __launch_bounds__(SEL_BLOCK) void select_smallest_kernel(const float *__restrict__ loss,
                                                                    int64_t n, int64_t k,
                                                                    float *__restrict__ mask_w) {
    select_smallest_block(loss, n, k, [](float x) { return x; },
                          [&](int64_t i, float, bool keep) { mask_w[i] = keep ? 1.0f : 0.0f; });
}

}  // namespace rlvi

using namespace rlvi;

extern "C" int rlvi_select_smallest_f32(const float *loss, int64_t n, int64_t k, float *mask_w,
                                        void *stream) {
    if (!loss || !mask_w) return RLVI_E_NULL;
    if (n < 0 || k < 0) return RLVI_E_SHAPE;
    if (n >= (int64_t)1 << 31) return RLVI_E_LIMIT;
    if (((uintptr_t)loss & 3) || ((uintptr_t)mask_w & 3)) return RLVI_E_ALIGN;
    if (n == 0) return 0;
    return launch(select_smallest_kernel, dim3(1), dim3(SEL_BLOCK), 0, static_cast<hipStream_t>(stream),
                  loss, n, k, mask_w);
}
