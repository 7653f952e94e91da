"""MI355X mirror of the small-loss baseline deep-learning/methods/train_jocor.py.

Same names, argument order and return types: kl_loss_compute(pred, soft_targets, reduce='none') (reference :17-26),
loss_jocor(y_1, y_2, t, forget_rate, ind, co_lambda=0.1) -> loss (:29-43) and
train_jocor(train_loader, epoch, model1, model2, optimizer, rate_schedule) -> train_acc1 (:46-76), the two models
trained through ONE optimizer over both parameter lists (main.py:228-231).

The reference runs two log_softmax, two softmax, two kl_div and two cross_entropy over the [B, C] blocks, moves
loss_pick to the host (.cpu(), a device sync), argsorts it there and averages the kept rows; here the joint loss,
the selection and the mean are pass 1 + a one-workgroup selection kernel, and the backward into both blocks is one
more pass (ops.jocor_loss, rlvi_amd/csrc/jocor.hip).  Kept as the reference runs it: kl_loss_compute(...,
reduce='none') tests `if reduce:`, which the string 'none' passes, so the KL terms are batch means -- one scalar
each, added to every row's loss_pick -- and every row, selected or not, receives their gradient.  The loss is a
0-dim tensor on the logits' device (the reference's is a CPU tensor): train_jocor only calls .backward() on it.
"""
import torch

from .. import ops

__all__ = ['train_jocor']

DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def kl_loss_compute(pred, soft_targets, reduce='none'):
    """mean_b KL(softmax(soft_targets_b) || softmax(pred_b)) as a 0-dim fp32 device tensor: the value the reference's
    truthy `reduce` (its only use, :33-34) returns -- pass 1 of the JoCoR kernels, forward only (loss_jocor takes
    the gradient of both KL terms inside ops.jocor_loss).  The per-row form (a falsy reduce) is not provided."""
    if not reduce:
        raise NotImplementedError("kl_loss_compute: only the batch mean (a truthy reduce, as the reference calls it)")
    z1, z2, t = ops._jocor_blocks(pred.detach(), soft_targets.detach(),
                                  torch.zeros(pred.shape[0], dtype=torch.int64, device=pred.device))
    out, _, _ = ops.jocor_forward(z1, z2, t, 0)
    return out[1].clone()


def loss_jocor(y_1, y_2, t, forget_rate, ind, co_lambda=0.1):
    return ops.jocor_loss(y_1, y_2, t, forget_rate, co_lambda=co_lambda)


def train_jocor(train_loader, epoch, model1, model2, optimizer, rate_schedule):
    hits = torch.zeros((), device=DEVICE)
    train_total = 0
    ws = None
    for (images, labels, indexes) in train_loader:
        images = images.to(DEVICE)
        labels = labels.to(DEVICE)
        logits1 = model1(images)
        logits2 = model2(images)
        ws = ws or ops.workspace(logits1.device)
        out = torch.empty(4, dtype=torch.float32, device=logits1.device)
        # (:68) with accuracy(logits1)[0] (:58-60) on the side: out[3] is the top-1 % of model 1 on this batch;
        # a label out of range is reported once, at the end of the epoch
        loss_1 = ops.jocor_loss(logits1, logits2, labels, rate_schedule[epoch], ws=ws, out=out, check=False)
        hits += out[3]
        train_total += 1
        optimizer.zero_grad()
        loss_1.backward()
        optimizer.step()
    if ws is not None:
        ws.raise_on_status("train_jocor")
    return float(hits) / float(train_total)
