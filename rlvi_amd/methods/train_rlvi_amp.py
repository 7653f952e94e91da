"""RLVI epoch with loss scaling for fp16 mixed precision (torch.amp.GradScaler).

    train_rlvi_amp(train_loader, model, optimizer, residuals, weights, overfit, threshold, scaler)
        -> (train_acc: float, threshold)

The reference's train_rlvi owns the backward (`logits.backward(grad)`), so a caller has no place to apply a
scaler; this is train_rlvi with one more argument and the same epoch body.  Per batch the scaler's current scale
is taken as a device tensor (`scaler.scale(one)`: no host sync), the fp16 M-step kernel multiplies the gradient by
it before its one rounding to fp16 (an overflow becomes inf, which the scaler's check catches), then
`scaler.step(optimizer)` and `scaler.update()` run as in any AMP loop.  Loss, residuals, pi and train_acc never
see the scale.  fp32 / bf16 logits, or a disabled scaler, keep stock AMP semantics: the gradient is multiplied by
the scale tensor in place.
"""
from .train_rlvi import _train_epoch

__all__ = ['train_rlvi_amp']


def train_rlvi_amp(train_loader, model, optimizer, residuals, weights, overfit, threshold, scaler):
    """train_rlvi (reference train_rlvi.py:52-106) with a torch.amp.GradScaler: one epoch, typically under
    torch.autocast("cuda", dtype=torch.float16).  Returns (train_acc, threshold) as train_rlvi does."""
    return _train_epoch(train_loader, model, optimizer, residuals, weights, overfit, threshold, scaler=scaler)
