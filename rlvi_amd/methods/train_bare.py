"""MI355X mirror of the baseline deep-learning/methods/train_bare.py (BARE: batch-statistics pruning).

Same names and argument order: class WeightedCCE(k=1, num_class=10, reduction="mean") with
forward(prediction, target_label, one_hot=True) (reference :15-57) and
train_bare(train_loader, model, optimizer, num_classes) -> train_acc (:60-82).

The reference runs about fifteen eager ops over the [B, C] block -- softmax, clamp, one-hot, mean and std down the
batch, two matmuls against the one-hot block, where, index_select twice, argmax, a second cross_entropy -- and reads
len(prun_idx) on the host.  Here the statistics, the selection and the loss are ops.bare_loss (rlvi_amd/csrc/bare.hip):
one launch for the reference's own batch sizes, two plus the M-step's gradient pass for large ones, no host sync.

forward returns the 0-dim scalar that the reference's `loss.mean()` yields: for reduction="mean" the loss itself, for
reduction="none" the mean of the per-row vector (train_bare's use, :64 and :78) -- the same number.  The vector
itself is not provided: its length is the number of kept rows, which depends on the data, so handing it out would
force a host sync per batch (the reference's len(prun_idx)).  Any other reduction raises NotImplementedError, and so
does one_hot=False, which is a NameError in the reference (y_true is only bound under `if one_hot:`).
"""
import torch
from torch import nn

from .. import ops

__all__ = ['train_bare']

DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class WeightedCCE(nn.Module):
    """BARE's pruned cross-entropy on the device (see the module docstring); attributes k, num_class, reduction."""

    def __init__(self, k=1, num_class=10, reduction="mean"):
        super().__init__()
        self.k, self.num_class, self.reduction = k, num_class, reduction

    def forward(self, prediction, target_label, one_hot=True):
        if not one_hot:
            raise NotImplementedError("WeightedCCE: one_hot=False is a NameError in the reference")
        return self.loss(prediction, target_label)

    def loss(self, prediction, target_label, ws=None, out=None, check=True):
        """forward with the plumbing of a training loop: the workspace, an fp32[4] device tensor that receives {L,
        n_kept, fallback, top-1 %}, and check=False to leave the label check to the end of the epoch."""
        if self.reduction not in ("mean", "none"):
            raise NotImplementedError(f"WeightedCCE: reduction={self.reduction!r} (only 'mean' and 'none', whose "
                                      "loss.mean() is the same scalar)")
        if prediction.shape[1] != self.num_class:
            raise ValueError(f"WeightedCCE(num_class={self.num_class}) on logits with {prediction.shape[1]} columns")
        return ops.bare_loss(prediction, target_label, k=self.k, ws=ws, out=out, check=check)


def train_bare(train_loader, model, optimizer, num_classes):
    hits = torch.zeros((), device=DEVICE)
    train_total = 0
    ws = None

    loss_fn = WeightedCCE(k=1, num_class=num_classes, reduction="none")
    for (images, labels, indexes) in train_loader:
        images = images.to(DEVICE)
        labels = labels.to(DEVICE)

        logits = model(images)
        ws = ws or ops.workspace(logits.device)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        # (:76) with accuracy(logits, labels)[0] (:72) on the side: out[3] is the top-1 % of this batch; a label out
        # of range is reported once, at the end of the epoch
        loss = loss_fn.loss(logits, labels, ws=ws, out=out, check=False)
        hits += out[3]
        train_total += 1
        optimizer.zero_grad()
        loss.mean().backward()
        optimizer.step()

    if ws is not None:
        ws.raise_on_status("train_bare")
    return float(hits) / float(train_total)
