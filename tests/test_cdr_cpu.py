"""CDR (deep-learning/methods/train_cdr.py) without a GPU: golden set G13 against a numpy restatement of the masking
lines, the mirror's interface against the reference's, the host-side table builder and argument checks of the C
entries, and the mirror's train_cdr on the CPU (a stand-in for the two ops it uses) against the reference's epochs.

The restatement (`restate`) is the whole claim of rlvi_amd/csrc/cdr.hip: the threshold is an exact order statistic,
    thr = np.partition(metric, total - nz)[total - nz],   metric = |g * v| over all covered tensors,
and the masked gradient is ((|v * g| >= thr).astype(f32) * f32(clip)) * g.  It must equal the reference's outputs
BIT FOR BIT on every case of G13 -- no case is left out.  The GPU tests (test_cdr_gpu.py) import it.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

from rlvi_amd import ops, synth
from rlvi_amd.methods import train_cdr  # noqa: F401  (the mirror these tests pin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(ROOT, "tests", "golden", "g13_cdr.npz")
LOOP = dict(seed=1313, N=256, B=64, D=16, H=32, C=10, epochs=3, lr=0.05, momentum=0.9, weight_decay=1e-4)


def restate(vs, gs, nz, clip):
    """train_cdr.py:22-44 on lists of fp32 arrays: (thr fp32, kept, masked gradients)."""
    metric = np.concatenate([np.abs(g.ravel() * v.ravel()) for v, g in zip(vs, gs)])
    assert metric.dtype == np.float32
    total = metric.size
    if not 1 <= nz <= total:
        raise IndexError("nz out of range")
    thr = np.partition(metric, total - nz)[total - nz]
    masked = [((np.abs(v * g) >= thr).astype(np.float32) * np.float32(clip)) * g for v, g in zip(vs, gs)]
    return np.float32(thr), int((metric >= thr).sum()), masked


def golden():
    return np.load(G13)


def case_inputs(g, key):
    """(vs, gs, ratio, clip) of a G13 case: the covered tensors split out of the stored concatenation."""
    cuts = np.cumsum(g[key + "/sizes"])[:-1]
    ratio, clip = g[key + "/real"]
    return np.split(g[key + "/v"], cuts), np.split(g[key + "/g"], cuts), ratio, clip


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_reproduces_every_reference_case_bit_for_bit():
    g = golden()
    keys = list(g["cases"])
    assert len(keys) == 13
    for key in keys:
        vs, gs, ratio, clip = case_inputs(g, key)
        total = sum(v.size for v in vs)
        nz = ops.cdr_num_nonzero(ratio, total)
        assert nz == int(g[key + "/nz"]), key                    # the mirror's nz is the reference's
        thr, kept, masked = restate(vs, gs, nz, clip)
        assert bits(thr) == bits(g[key + "/thr"]), key
        assert kept == int(g[key + "/kept"]), key
        assert np.array_equal(bits(np.concatenate(masked)), bits(g[key + "/masked"])), key
        # tensors of other ranks went through the reference's step untouched
        assert np.array_equal(bits(g[key + "/uncovered_g"]), bits(g[key + "/uncovered_at_step"])), key


def test_fixture_size_and_contents():
    assert os.path.getsize(G13) < 500 * 1024
    g = golden()
    keys = list(g["cases"])
    for kind in ("mlp", "convbn"):
        for r in ("1.0", "0.8", "0.5", "nz3", "nz1"):
            assert f"{kind}_{r}" in keys
        assert int(g[kind + "_nz1/nz"]) == 1 and int(g[kind + "_nz3/nz"]) == 3
        assert int(g[kind + "_1.0/nz"]) == int(g[kind + "_1.0/sizes"].sum())
        assert g[kind + "_0.5/uncovered_g"].size > 0
    assert int(g["built_ties/kept"]) > int(g["built_ties/nz"])
    assert float(g["built_zeros/thr"]) == 0 and int(g["built_zeros/kept"]) == int(g["built_zeros/sizes"].sum())
    m = np.abs(g["built_binade/g"] * g["built_binade/v"])
    assert m.min() >= 1 and m.max() < 2
    # dropped entries of negative gradients are negative zeros in the reference: the fixture can tell m * g from a
    # select that writes +0
    dropped = g["built_ties/masked"][np.signbit(g["built_ties/g"]) & (g["built_ties/masked"] == 0)]
    assert dropped.size and np.signbit(dropped).all()
    assert g["loop/params"].shape[0] == 3 and g["loop/train_acc"].shape == (3,)
    assert g["loop/rate_schedule"][0] == 0                      # epoch 0: clip == 1


def test_names_argument_order_and_all_match_the_reference():
    import importlib
    g = golden()
    cd = importlib.import_module("rlvi_amd.methods.train_cdr")
    assert list(cd.__all__) == list(g["ref/all"]) == ['train_cdr']
    for fn in ("train_one_step", "train_cdr"):
        ps = list(inspect.signature(getattr(cd, fn)).parameters.values())
        positional = [q for q in ps if q.kind is not q.KEYWORD_ONLY]
        mine = [q.name if q.default is q.empty else f"{q.name}={q.default!r}" for q in positional]
        assert mine == list(g["ref/sig/" + fn]), fn
        extra = [(q.name, q.default) for q in ps if q.kind is q.KEYWORD_ONLY]
        assert extra == ([("reuse_forward", False)] if fn == "train_cdr" else []), fn
    import rlvi_amd.methods as methods
    assert methods.train_cdr is cd.train_cdr


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


def fill(lib, v, g, n, buf=None):
    nseg = len(n)
    nbytes = lib.rlvi_cdr_table_bytes(nseg)
    raw = (ctypes.c_char * (nbytes + 16))()
    host = ctypes.addressof(raw) + (-ctypes.addressof(raw) % 16) if buf is None else buf
    total, chunks = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = lib.rlvi_cdr_table_fill(host, (ctypes.c_void_p * nseg)(*v), (ctypes.c_void_p * nseg)(*g),
                                 (ctypes.c_int64 * nseg)(*n), nseg, ctypes.byref(total), ctypes.byref(chunks))
    table = None
    if rc == 0:
        table = np.frombuffer(ctypes.string_at(host, nbytes), np.int64).reshape(nseg + 1, 4)
    return rc, total.value, chunks.value, table


def test_table_fill_chunk_prefix_totals_and_errors(lib):
    from rlvi_amd import _lib
    for name in ("rlvi_cdr_table_bytes", "rlvi_cdr_table_fill", "rlvi_cdr_scratch_bytes", "rlvi_cdr_mask_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.rlvi_abi_version() == 3
    assert lib.rlvi_cdr_table_bytes(0) == 0 and lib.rlvi_cdr_scratch_bytes(0) == 0
    assert lib.rlvi_cdr_table_bytes(5) > lib.rlvi_cdr_table_bytes(4) > 0 and lib.rlvi_cdr_scratch_bytes(4) > 0
    # the chunk size, from one large segment
    rc, total, chunks, _ = fill(lib, [0x1000], [0x2000], [1 << 20])
    assert rc == 0 and total == 1 << 20 and (1 << 20) % chunks == 0
    ch = (1 << 20) // chunks
    n = [1, ch - 1, ch, ch + 1, 5 * ch + 3, 7, 3 * ch]
    v = [0x10000 + 4 * i for i in range(len(n))]               # 4-byte alignment is enough
    gp = [0x900000 + 4 * (3 * i + 1) for i in range(len(n))]
    rc, total, chunks, t = fill(lib, v, gp, n)
    assert rc == 0 and total == sum(n)
    per = [-(-x // ch) for x in n]
    assert chunks == sum(per)
    assert list(t[:-1, 0]) == v and list(t[:-1, 1]) == gp and list(t[:-1, 2]) == n
    assert list(t[:, 3]) == [0] + list(np.cumsum(per))          # the chunk prefix, closed by the number of chunks
    # errors, all on the host
    assert fill(lib, [0x1000, 0], [0x2000, 0x3000], [4, 4])[0] == -1            # a null segment pointer
    assert fill(lib, [0x1000], [0x2000], [4], buf=0)[0] == -1                   # no host buffer
    assert fill(lib, [0x1000, 0x1100], [0x2000, 0x2100], [4, 0])[0] == -2       # n < 1
    assert fill(lib, [0x1000, 0x1100], [0x2000, 0x2100], [-3, 4])[0] == -2
    assert fill(lib, [0x1002], [0x2000], [4])[0] == -3                          # not 4-byte aligned
    assert fill(lib, [0x1000], [0x2001], [4])[0] == -3
    nul = ctypes.c_int64(0)
    raw = (ctypes.c_char * 256)()
    assert lib.rlvi_cdr_table_fill(ctypes.addressof(raw), None, None, None, 0, ctypes.byref(nul),
                                   ctypes.byref(nul)) == -1
    one = (ctypes.c_void_p * 1)(0x1000)
    assert lib.rlvi_cdr_table_fill(ctypes.addressof(raw), one, one, (ctypes.c_int64 * 1)(4), 0, ctypes.byref(nul),
                                   ctypes.byref(nul)) == -2                     # nseg < 1


def test_mask_argument_errors_without_a_gpu(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255
    sb = lib.rlvi_cdr_scratch_bytes(3)
    f = lib.rlvi_cdr_mask_f32
    #   table nseg total chunks nz clip scratch scratch_bytes thr kept stream
    assert f(None, 3, 100, 3, 50, 0.5, p, sb, p, p, None) == -1
    assert f(p, 3, 100, 3, 50, 0.5, None, sb, p, p, None) == -1
    assert f(p, 3, 100, 3, 50, 0.5, p, sb, None, p, None) == -1
    assert f(p, 3, 100, 3, 50, 0.5, p, sb, p, None, None) == -1
    assert f(p, 0, 100, 3, 50, 0.5, p, sb, p, p, None) == -2                    # nseg < 1
    assert f(p, 3, 100, 3, 0, 0.5, p, sb, p, p, None) == -2                     # nz < 1
    assert f(p, 3, 100, 3, -4, 0.5, p, sb, p, p, None) == -2
    assert f(p, 3, 100, 3, 101, 0.5, p, sb, p, p, None) == -2                   # nz > total
    assert f(p, 3, 100, 2, 50, 0.5, p, sb, p, p, None) == -2                    # fewer chunks than segments
    assert f(p + 8, 3, 100, 3, 50, 0.5, p, sb, p, p, None) == -3                # table not 16-byte aligned
    assert f(p, 3, 100, 3, 50, 0.5, p + 4, sb, p, p, None) == -3
    assert f(p, 3, 100, 3, 50, 0.5, p, sb, p + 2, p, None) == -3
    assert f(p, 3, 100, 3, 50, 0.5, p, sb, p, p + 4, None) == -3
    assert f(p, 3, 100, 3, 50, 0.5, p, sb - 1, p, p, None) == -4                # scratch too small
    assert f(p, 3, 1 << 32, 3, 50, 0.5, p, sb, p, p, None) == -5


def test_nz_is_the_reference_expression_and_zero_raises_index_error():
    for total in (352, 507, 11_173_962):
        for r in (1.0, 0.8, 0.5, np.float64(0.7), 1 - np.float64(0.3), 3.5 / total, np.float32(0.25)):
            assert ops.cdr_num_nonzero(r, total) == int(r * total)
    with pytest.raises(IndexError):
        ops.cdr_num_nonzero(0.0, 352)
    with pytest.raises(IndexError):
        ops.cdr_num_nonzero(0.9 / 352, 352)
    with pytest.raises(IndexError):
        restate([np.ones(4, np.float32)], [np.ones(4, np.float32)], 0, 1.0)


def test_cpu_tensors_are_refused(lib):
    import torch
    from rlvi_amd import _lib
    w = torch.nn.Parameter(torch.ones(3, 4))
    w.grad = torch.ones(3, 4)
    with pytest.raises(_lib.RlviError, match="no CPU fallback"):
        ops.CdrMasker([w])
    with pytest.raises(_lib.RlviError, match="no CPU fallback"):
        ops.cdr_mask_([w], 0.5, 0.5)


class CpuOps:
    """Local stand-in for the two ops train_cdr uses, on CPU tensors: the masker is the numpy restatement above, the
    top-1 % is accuracy()'s own torch ops in its order (deep-learning/utils.py:65-79)."""

    class CdrMasker:
        def __init__(self, params):
            self.params = [p for p in params if p.dim() in (2, 4)]
            self.total = sum(p.numel() for p in self.params)

        def __call__(self, nonzero_ratio, clip):
            import torch
            nz = ops.cdr_num_nonzero(nonzero_ratio, self.total)
            vs = [p.detach().numpy() for p in self.params]
            gs = [p.grad.detach().numpy() for p in self.params]
            thr, kept, masked = restate(vs, gs, nz, clip)
            for p, m in zip(self.params, masked):
                p.grad = torch.from_numpy(m)
            return torch.tensor(thr), torch.tensor(kept)

    @staticmethod
    def evaluate_batch(logits, labels, out=None, ws=None):
        import torch
        import torch.nn.functional as F
        output = F.softmax(logits, dim=1)
        _, pred = output.topk(5, 1, True, True)
        correct = pred.t().eq(labels.view(1, -1).expand_as(pred.t()))
        prec1 = correct[:1].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / labels.size(0))
        return torch.stack([torch.zeros(()), prec1[0], torch.zeros(()), torch.zeros(())])


def loop_setup(device=None):
    import torch
    from torch import nn
    g, p = golden(), LOOP
    X, y = synth.jocor_loop_inputs(p["seed"], p["N"], p["D"], p["C"])
    loader = [(torch.from_numpy(X[s:s + p["B"]]), torch.from_numpy(y[s:s + p["B"]]),
               torch.arange(s, min(s + p["B"], p["N"]))) for s in range(0, p["N"], p["B"])]
    model = nn.Sequential(nn.Linear(p["D"], p["H"]), nn.ReLU(), nn.Linear(p["H"], p["C"]))
    init, off = g["loop/init"], 0
    with torch.no_grad():
        for q in model.parameters():
            q.copy_(torch.from_numpy(init[off:off + q.numel()].reshape(q.shape)))
            off += q.numel()
    if device is not None:
        model = model.to(device)
    opt = torch.optim.SGD(model.parameters(), lr=p["lr"], momentum=p["momentum"], weight_decay=p["weight_decay"])
    model.train()
    return g, loader, model, opt


def flat(model):
    return np.concatenate([q.detach().cpu().numpy().ravel() for q in model.parameters()])


@pytest.mark.parametrize("reuse_forward", [False, True])
def test_mirror_loop_on_the_cpu_equals_the_reference_exactly(reuse_forward, monkeypatch):
    """The mirror's statements with the stand-in ops are the reference's torch CPU ops in the reference's order, on
    one thread: parameters and accuracies equal G13's bit for bit.  reuse_forward=True skips the first forward; this
    model has neither dropout nor BatchNorm, so it takes the same parameters to the same accuracies (the logits of
    both forwards are the same numbers)."""
    import torch
    cd = sys.modules["rlvi_amd.methods.train_cdr"]
    monkeypatch.setattr(cd, "ops", CpuOps)
    monkeypatch.setattr(cd, "DEVICE", torch.device("cpu"))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        g, loader, model, opt = loop_setup()
        rs = g["loop/rate_schedule"]
        for e in range(LOOP["epochs"]):
            acc = cd.train_cdr(loader, e, model, opt, rs, reuse_forward=reuse_forward)
            assert acc == g["loop/train_acc"][e], (e, acc)
            assert np.array_equal(bits(flat(model)), bits(g["loop/params"][e])), f"epoch {e}"
    finally:
        torch.set_num_threads(threads)
