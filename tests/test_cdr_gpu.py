"""CDR's gradient masking on the MI355X (run with -m gpu): ops.CdrMasker and methods.train_cdr against golden set G13
(the reference's own outputs) and the numpy restatement of test_cdr_cpu -- bit for bit: the threshold is an exact
order statistic and the mask one multiply, so there is no tolerance anywhere except against G13's loop, whose forward
and backward ran in CPU arithmetic.
"""
import sys

import numpy as np
import pytest

from test_cdr_cpu import LOOP, bits, case_inputs, flat, golden, loop_setup, restate

pytestmark = pytest.mark.gpu

CASES = list(golden()["cases"])


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rlvi_amd import _lib, ops
    _lib.load()
    return torch, ops, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_process_state_left_behind():
    """No test leaves a knob set, a sticky status or accumulate-mode records behind (later tests would see them)."""
    yield
    import torch
    if not torch.cuda.is_available():
        return
    from rlvi_amd import _lib, ops
    left = [n for n in _lib.tune_overrides() if n != "RLVI_DEVICE_SHARERS"]
    for name in left:
        _lib.load().rlvi_tune_unset(name.encode())
    torch.cuda.synchronize()
    dirty = []
    for key, ws in list(ops._workspaces.items()):
        st = ws.status()
        if st:
            ws.clear_status()
            dirty.append(f"workspace {key}: sticky status {st}")
        if ws.pending_records():
            ops.mstep_reduce(ws=ws)
            dirty.append(f"workspace {key}: accumulate-mode records without an epoch end")
    assert not left, f"knobs left set by this test: {left}"
    assert not dirty, "; ".join(dirty)


def as_params(torch, dev, vs, gs, pad=0):
    """Parameters [1, n] that are VIEWS into one buffer each for v and g, tensor after tensor with `pad` elements
    between them, so that their addresses are whatever the sizes make them (4-byte aligned, often no more)."""
    sizes = [v.size for v in vs]
    offs = np.concatenate([[0], np.cumsum([s + pad for s in sizes])[:-1]]).astype(np.int64)
    room = int(offs[-1] + sizes[-1])
    vbuf = torch.zeros(room, device=dev)
    gbuf = torch.zeros(room + 1, device=dev)[1:]               # g and v at different offsets from a 16-byte boundary
    params = []
    for v, g, o, n in zip(vs, gs, offs, sizes):
        vbuf[o:o + n] = torch.from_numpy(np.ascontiguousarray(v).ravel()).to(dev)
        gbuf[o:o + n] = torch.from_numpy(np.ascontiguousarray(g).ravel()).to(dev)
        p = torch.nn.Parameter(vbuf[o:o + n].view(1, n), requires_grad=True)
        p.grad = gbuf[o:o + n].view(1, n)
        assert p.data_ptr() == vbuf.data_ptr() + 4 * o
        params.append(p)
    return params, gbuf


def check_against(torch, params, thr, kept, vs, gs, nz, clip, what=""):
    r_thr, r_kept, r_masked = restate([v.ravel() for v in vs], [g.ravel() for g in gs], nz, clip)
    torch.cuda.synchronize()
    assert bits(thr.cpu().numpy()) == bits(r_thr), (what, float(thr), float(r_thr))
    assert int(kept) == r_kept, (what, int(kept), r_kept)
    for i, (p, m) in enumerate(zip(params, r_masked)):
        mine = p.grad.detach().cpu().numpy().ravel()
        diff = int((bits(mine) != bits(m)).sum())
        assert diff == 0, f"{what}: tensor {i} of {len(params)}: {diff} of {m.size} entries differ"


@pytest.mark.parametrize("key", CASES)
def test_every_reference_case_bit_for_bit(key, gpu):
    torch, ops, dev = gpu
    g = golden()
    vs, gs, ratio, clip = case_inputs(g, key)
    params, _ = as_params(torch, dev, vs, gs)
    bias = torch.nn.Parameter(torch.zeros(max(g[key + "/uncovered_g"].size, 1), device=dev))
    unc = np.resize(g[key + "/uncovered_g"], bias.numel()).astype(np.float32)
    bias.grad = torch.from_numpy(unc).to(dev)
    masker = ops.CdrMasker(params[:1] + [bias] + params[1:])
    assert masker.nseg == len(params) and masker.total == sum(v.size for v in vs)
    thr, kept = masker(ratio, clip)
    torch.cuda.synchronize()
    assert thr.dtype == torch.float32 and kept.dtype == torch.int64 and thr.is_cuda and kept.is_cuda
    assert bits(thr.cpu().numpy()) == bits(g[key + "/thr"])
    assert int(kept) == int(g[key + "/kept"])
    mine = np.concatenate([p.grad.cpu().numpy().ravel() for p in params])
    assert np.array_equal(bits(mine), bits(g[key + "/masked"]))
    assert np.array_equal(bits(bias.grad.cpu().numpy()), bits(unc))           # other ranks: untouched


def resnet18_tensors(torch, seed=18):
    from rlvi_amd import driver
    torch.manual_seed(seed)
    model = driver.ResNet18()
    vs = [p.detach().numpy().copy() for _, p in model.named_parameters() if p.dim() in (2, 4)]
    rng = np.random.default_rng(seed)
    # gradients spread over many binades, as a network's are
    gs = [(rng.standard_normal(v.shape) * np.exp(2 * rng.standard_normal(v.shape)) * 1e-3).astype(np.float32)
          for v in vs]
    return vs, gs


def test_resnet18_parameter_list(gpu):
    torch, ops, dev = gpu
    vs, gs = resnet18_tensors(torch)
    total = sum(v.size for v in vs)
    assert 11_100_000 < total < 11_250_000
    params = []
    for v, g in zip(vs, gs):
        p = torch.nn.Parameter(torch.from_numpy(v).to(dev))
        p.grad = torch.from_numpy(g).to(dev)
        params.append(p)
    masker = ops.CdrMasker(params)
    for ratio in (0.7, 0.5):
        for p, g in zip(params, gs):
            p.grad.copy_(torch.from_numpy(g))
        thr, kept = masker(ratio, ratio)
        check_against(torch, params, thr, kept, vs, gs, int(ratio * total), ratio, f"ResNet18 ratio {ratio}")
    assert masker.uploads == 1


def test_200_segments_at_odd_offsets(gpu):
    torch, ops, dev = gpu
    rng = np.random.default_rng(200)
    sizes = np.concatenate([[1, 2, 3, 4, 5, 4095, 4096, 4097, 5000], rng.integers(1, 5001, 191)])
    vs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    gs = [(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2)).astype(np.float32) for n in sizes]
    total = int(sizes.sum())
    for pad, ratio in ((0, 0.6), (1, 0.013), (3, 0.9)):
        params, _ = as_params(torch, dev, vs, gs, pad=pad)
        assert len({p.data_ptr() % 16 for p in params}) == 4
        thr, kept = ops.cdr_mask_(params, ratio, 0.4)
        check_against(torch, params, thr, kept, vs, gs, int(ratio * total), 0.4, f"pad {pad}")


def test_one_segment_beyond_the_infinity_cache(gpu):
    torch, ops, dev = gpu
    n = 64 * 1024 * 1024                                        # v and g: 512 MiB together
    rng = np.random.default_rng(64)
    v = rng.standard_normal(n, dtype=np.float32)
    g = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
    p = torch.nn.Parameter(torch.from_numpy(v).to(dev).view(1, n))
    p.grad = torch.from_numpy(g).to(dev).view(1, n)
    thr, kept = ops.cdr_mask_([p], 0.8, 0.8)
    check_against(torch, [p], thr, kept, [v], [g], int(0.8 * n), 0.8, "64 M")


def edge_case(name):
    rng = np.random.default_rng(77)
    sizes = (5000, 333, 8192, 1)
    if name == "all_equal":
        vs = [np.full(n, 1.5, np.float32) for n in sizes]
        gs = [np.where(rng.random(n) < 0.5, 2.0, -2.0).astype(np.float32) for n in sizes]
    elif name == "denormals":
        vs = [np.full(n, 1e-20, np.float32) for n in sizes]
        gs = [(rng.standard_normal(n) * 1e-20).astype(np.float32) for n in sizes]
    else:
        vs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
        gs = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    if name == "inf":
        vs[0][17] = 0.5                                         # (a non-zero weight: inf * 0 would be a NaN metric)
        gs[0][17] = -np.inf
    return vs, gs


@pytest.mark.parametrize("name,ratio", [("all_equal", 0.5), ("denormals", 0.5), ("inf", 0.3), ("plain", "total"),
                                        ("plain", "one"), ("inf", "one")])
def test_edges_vs_restatement(name, ratio, gpu):
    torch, ops, dev = gpu
    vs, gs = edge_case(name)
    total = sum(v.size for v in vs)
    if ratio == "total":
        ratio = 1.0
    elif ratio == "one":
        ratio = 1.5 / total
    nz = int(ratio * total)
    if name == "denormals":
        m = np.concatenate([np.abs(g * v) for v, g in zip(vs, gs)])
        assert 0 < m.max() < np.finfo(np.float32).tiny          # every metric is a denormal or zero
    params, _ = as_params(torch, dev, vs, gs)
    thr, kept = ops.cdr_mask_(params, ratio, 0.25)
    check_against(torch, params, thr, kept, vs, gs, nz, 0.25, name)
    if name == "all_equal":
        assert int(kept) == total
    if name == "inf":
        assert np.isinf(params[0].grad[0, 17].item())


def test_nz_zero_raises_index_error_and_bad_inputs_raise(gpu):
    torch, ops, dev = gpu
    vs, gs = edge_case("plain")
    params, _ = as_params(torch, dev, vs, gs)
    masker = ops.CdrMasker(params)
    before = [p.grad.clone() for p in params]
    with pytest.raises(IndexError):
        masker(0.0, 1.0)
    assert all(torch.equal(a, p.grad) for a, p in zip(before, params))
    params[1].grad = None
    with pytest.raises(ValueError, match="no gradient"):
        masker(0.5, 0.5)
    w = torch.nn.Parameter(torch.ones(6, 8, device=dev))
    w.grad = torch.ones(8, 6, device=dev).t()
    with pytest.raises(ValueError, match="contiguous"):
        ops.CdrMasker([w])(0.5, 0.5)
    with pytest.raises(TypeError):
        ops.CdrMasker([torch.nn.Parameter(torch.ones(6, 8, device=dev, dtype=torch.float16))])


def test_two_calls_give_identical_bytes(gpu):
    torch, ops, dev = gpu
    vs, gs = resnet18_tensors(torch, seed=19)
    vs, gs = vs[:20], gs[:20]
    params, gbuf = as_params(torch, dev, vs, gs)
    g0 = gbuf.clone()
    masker = ops.CdrMasker(params)
    outs = []
    for _ in range(2):
        gbuf.copy_(g0)
        thr, kept = masker(0.55, 0.55)
        outs.append((thr.clone(), kept.clone(), gbuf.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][2].view(torch.int32), outs[1][2].view(torch.int32))


def test_table_is_uploaded_only_when_a_pointer_changed(gpu):
    torch, ops, dev = gpu
    vs, gs = edge_case("plain")
    params = []
    for v, g in zip(vs, gs):
        p = torch.nn.Parameter(torch.from_numpy(v).to(dev).view(1, -1))
        p.grad = torch.from_numpy(g).to(dev).view(1, -1)
        params.append(p)
    masker = ops.CdrMasker(params)
    assert masker.uploads == 0
    masker(0.5, 0.5)
    assert masker.uploads == 1
    masker(0.5, 0.5)
    masker(0.9, 0.9)
    assert masker.uploads == 1                                  # same addresses: the table stays
    old = params[2].grad                                        # (kept alive: the allocator must hand out another block)
    params[2].grad = torch.from_numpy(gs[2]).to(dev).view(1, -1)
    assert params[2].grad.data_ptr() != old.data_ptr()
    for p, g in zip(params, gs):
        p.grad.copy_(torch.from_numpy(g).view(1, -1))
    thr, kept = masker(0.5, 0.5)
    assert masker.uploads == 2
    check_against(torch, params, thr, kept, vs, gs, int(0.5 * masker.total), 0.5, "after a reallocation")


def test_capture_into_a_graph_and_replay(gpu):
    torch, ops, dev = gpu
    vs, gs = edge_case("plain")
    params, gbuf = as_params(torch, dev, vs, gs)
    g0 = gbuf.clone()
    masker = ops.CdrMasker(params)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        masker(0.6, 0.35)                                       # warm-up: the table is uploaded here, not in the graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        thr, kept = masker(0.6, 0.35)
    assert masker.uploads == 1
    total = masker.total
    for _ in range(2):
        gbuf.copy_(g0)
        thr.zero_()
        kept.zero_()
        graph.replay()
        check_against(torch, params, thr, kept, vs, gs, int(0.6 * total), 0.35, "graph replay")


def stock_one_step(torch, model, data, label, optimizer, criterion, nonzero_ratio, clip):
    """train_cdr.py:16-47 as stock torch ops on the model's device."""
    model.train()
    pred = model(data)
    loss = criterion(pred, label)
    loss.backward()
    to_concat_g, to_concat_v = [], []
    for name, param in model.named_parameters():
        if param.dim() in [2, 4]:
            to_concat_g.append(param.grad.data.view(-1))
            to_concat_v.append(param.data.view(-1))
    all_g, all_v = torch.cat(to_concat_g), torch.cat(to_concat_v)
    metric = torch.abs(all_g * all_v)
    nz = int(nonzero_ratio * all_v.size(0))
    top_values, _ = torch.topk(metric, nz)
    thresh = top_values[-1]
    masks = []
    for name, param in model.named_parameters():
        if param.dim() in [2, 4]:
            mask = (torch.abs(param.data * param.grad.data) >= thresh).type(torch.float32)
            masks.append(mask.bool().cpu().numpy().ravel())
            mask = mask * clip
            param.grad.data = mask * param.grad.data
    optimizer.step()
    optimizer.zero_grad()
    return pred, masks


def stock_train_cdr(torch, loader, epoch, model, optimizer, rate_schedule, dev, masks=None):
    import torch.nn.functional as F
    train_total, train_correct = 0, 0
    clip = 1 - rate_schedule[epoch]
    for (data, labels, indexes) in loader:
        data, labels = data.to(dev), labels.to(dev)
        logits = model(data)
        _, pred = F.softmax(logits, dim=1).topk(5, 1, True, True)
        correct = pred.t().eq(labels.view(1, -1).expand_as(pred.t()))
        train_correct += correct[:1].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / labels.size(0))
        train_total += 1
        _, m = stock_one_step(torch, model, data, labels, optimizer, torch.nn.CrossEntropyLoss(), clip, clip)
        if masks is not None:
            masks.append(np.concatenate(m))
    return float(train_correct) / float(train_total)


@pytest.mark.parametrize("reuse_forward", [False, True])
def test_train_cdr_equals_stock_torch_on_the_same_device(reuse_forward, gpu):
    """Both sides run the same forward and backward kernels, so the gradients agree, and the mask is exact:
    parameters bit-identical after every epoch, accuracies equal."""
    torch, ops, dev = gpu
    from rlvi_amd.methods import train_cdr
    g, loader, mine, opt_mine = loop_setup(dev)
    _, _, stock, opt_stock = loop_setup(dev)
    rs = g["loop/rate_schedule"]
    for e in range(LOOP["epochs"]):
        acc = train_cdr(loader, e, mine, opt_mine, rs, reuse_forward=reuse_forward)
        ref = stock_train_cdr(torch, loader, e, stock, opt_stock, rs, dev)
        assert acc == ref, (e, acc, ref)
        diff = int((bits(flat(mine)) != bits(flat(stock))).sum())
        assert diff == 0, f"epoch {e}: {diff} parameters differ from the stock-torch run"
    ops.workspace(dev).raise_on_status("train_cdr")


def test_train_cdr_three_epochs_vs_reference(gpu):
    """Against G13's loop (CPU arithmetic in forward and backward): the bar of test_jocor_gpu's loop.  A metric that
    sits within rounding of the threshold can fall on the other side of it here; the masks of every step are compared
    with a CPU twin of the reference's statements and the number of entries that differ is reported."""
    torch, ops, dev = gpu
    cd = sys.modules["rlvi_amd.methods.train_cdr"]
    g, loader, model, opt = loop_setup(dev)
    _, _, twin, opt_twin = loop_setup()
    rs = g["loop/rate_schedule"]
    mine_masks, twin_masks = [], []
    real = cd._masker

    def recording(m):
        masker = real(m)

        def call(ratio, clip):
            raw = [p.grad.clone() for p in masker.params]
            thr, kept = masker(ratio, clip)
            mine_masks.append(np.concatenate([(torch.abs(p.data * r) >= thr).cpu().numpy().ravel()
                                              for p, r in zip(masker.params, raw)]))
            return thr, kept
        return call
    cd._masker = recording
    try:
        for e in range(LOOP["epochs"]):
            acc = cd.train_cdr(loader, e, model, opt, rs)
            stock_train_cdr(torch, loader, e, twin, opt_twin, rs, torch.device("cpu"), masks=twin_masks)
            flips = sum(int((a != b).sum()) for a, b in zip(mine_masks, twin_masks))
            entries = sum(a.size for a in mine_masks)
            note = f"epoch {e}: {flips} of {entries} mask entries differ from the CPU twin so far"
            assert abs(acc - g["loop/train_acc"][e]) <= 1e-4, (acc, note)
            np.testing.assert_allclose(flat(model), g["loop/params"][e], rtol=1e-4, atol=1e-5, err_msg=note)
    finally:
        cd._masker = real
