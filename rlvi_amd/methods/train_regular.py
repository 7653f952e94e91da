"""MI355X mirror of the baseline deep-learning/methods/train_regular.py: plain cross-entropy.

Same name and argument order: train_regular(train_loader, model, optimizer) -> train_acc (reference :15-36).
F.cross_entropy (:30), its backward (:32) and the top-1 of accuracy(logits, labels) (:26) are ONE call of the
streaming M-step kernel with unit weights and 1 / B (ops.weighted_cross_entropy: no new kernel); the per-batch
percentages pile up on the device and are read once, at the end of the epoch.
"""
import torch

from .. import ops

__all__ = ['train_regular']

DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def train_regular(train_loader, model, optimizer):
    acc = torch.zeros((), device=DEVICE)
    train_total = 0
    ones = {}
    ws = None

    for (images, labels, indexes) in train_loader:
        images = images.to(DEVICE)
        labels = labels.to(DEVICE)

        logits = model(images)
        B = logits.shape[0]
        if B not in ones:
            ones[B] = torch.ones(B, dtype=torch.float32, device=logits.device)
        ws = ws or ops.workspace(logits.device, B, B)
        # (:30) mean CE = sum_i 1 * CE_i / B; out[1] is the top-1 % of this batch (:26)
        loss, out = ops.weighted_cross_entropy(logits, labels, None, ones[B], None)
        acc += out[1]
        train_total += 1
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

    if ws is not None:
        ws.raise_on_status("train_regular")
    return float(acc) / float(train_total)
