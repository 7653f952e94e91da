"""MI355X mirror of the gradient-masking baseline deep-learning/methods/train_cdr.py (CDR).

Same names, argument order and statement order: train_one_step(model, data, label, optimizer, criterion,
nonzero_ratio, clip) -> (float(acc[0]), loss) (reference :16-50) and train_cdr(train_loader, epoch, model, optimizer,
rate_schedule) -> train_acc (:53-72): the first forward for the accuracy (:62-63), model.train() inside
train_one_step (:17), the second forward, backward (:18-20), the mask (:22-44), step, zero_grad (:46-47), and
clip = 1 - rate_schedule[epoch] handed in as both ratio and clip (:57,:68).

CDR's cost is not in the loss: after backward the reference concatenates every covered gradient and parameter (two
copies of all weights), runs torch.topk over 50-100 % of them to read one number, and then masks tensor by tensor --
some five eager kernels each.  Here the threshold is an exact order statistic found by a radix descent over a table
of the tensors and the mask is one multiply pass (ops.CdrMasker, rlvi_amd/csrc/cdr.hip): five launches whatever the
network, the reference's masked gradients bit for bit.  The masker is kept per model; its table follows the
gradients' addresses (zero_grad() frees them every step).

train_cdr takes one keyword the reference has not: reuse_forward=True takes the accuracy from the logits of the
training forward and skips the first one.  The parameters then go the same way for a model without dropout, and
BatchNorm's running statistics are updated once per batch instead of twice; the default is the reference's two
forwards.
"""
import weakref

import torch
from torch import nn

from .. import ops

__all__ = ['train_cdr']

DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")

_maskers = weakref.WeakKeyDictionary()


def _masker(model):
    m = _maskers.get(model)
    if m is None:
        m = _maskers[model] = ops.CdrMasker([param for name, param in model.named_parameters()])
    return m


def _prec1(logits, labels):
    """accuracy(logits, labels, topk=(1, 5))[0] (deep-learning/utils.py:65-79) as a device scalar: the top-1 %."""
    with torch.no_grad():
        return ops.evaluate_batch(logits.detach(), labels)[1]


def _one_step(model, data, label, optimizer, criterion, nonzero_ratio, clip):
    model.train()
    pred = model(data)
    loss = criterion(pred, label)
    loss.backward()
    _masker(model)(nonzero_ratio, clip)                      # (:22-44)
    optimizer.step()
    optimizer.zero_grad()
    return pred, loss


def train_one_step(model, data, label, optimizer, criterion, nonzero_ratio, clip):
    pred, loss = _one_step(model, data, label, optimizer, criterion, nonzero_ratio, clip)
    return float(_prec1(pred, label)), loss                  # (:48-50)


def train_cdr(train_loader, epoch, model, optimizer, rate_schedule, *, reuse_forward=False):
    train_total = 0
    train_correct = torch.zeros((), device=DEVICE)

    clip = 1 - rate_schedule[epoch]
    criterion = nn.CrossEntropyLoss()
    for (data, labels, indexes) in train_loader:
        data = data.to(DEVICE)
        labels = labels.to(DEVICE)
        if not reuse_forward:
            logits = model(data)                             # (:62) in the mode the caller left the model in
            train_correct += _prec1(logits, labels)
        train_total += 1
        # train_one_step without its float(acc[0]): train_cdr drops that value (:67), and taking it is a host sync
        pred, loss = _one_step(model, data, labels, optimizer, criterion, clip, clip)
        if reuse_forward:
            train_correct += _prec1(pred, labels)

    train_acc = float(train_correct) / float(train_total)
    return train_acc
