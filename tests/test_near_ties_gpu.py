"""The E-step's stop decision on inputs built to sit near tol (golden set G11; run with -m gpu).

The trajectory solver decides the iteration count without always measuring the stop tests at the true
nodes: the fourth-order first round accepts on estimated step errors inside a band, a round whose
correction is small accepts when every test clears tol by a margin, and a correction at or below
TJ_ACCEPT is accepted outright (rlvi_traj.h, rlvi_trajb.h).  Every path that decides the count runs here on
every G11 case (tests/test_near_ties_cpu.py explains the cases and what "pinned" means):

  pinned      the reference's count, and pi within REL of the oracle's;
  not pinned  a count within the fp32 rounding of the stop tests (`feasible`: the fp32 and fp64 references
              straddle tol at every test it passes or stops on), and pi within REL of the oracle run to
              exactly that count (tol = 0, maxiter = count).
"""
import numpy as np
import pytest

from test_gpu_parity import gpu, no_process_state_left_behind, tune, untune  # noqa: F401  (fixtures)
from test_near_ties_cpu import g11_case, g11_cases, g11_meta, pinning
from test_oracle_golden import REL, rel_pi

pytestmark = pytest.mark.gpu

DRIFTS = (1.001, 1.01, 1.05, 1.30)


def entries():
    return sorted({g11_meta(k)["entry"] for k in g11_cases()})


def cases_of(entry):
    return [k for k in g11_cases() if g11_meta(k)["entry"] == entry]


_PIN = {}


def pin(c, oracle):
    if c["key"] not in _PIN:
        _PIN[c["key"]] = pinning(c["r"], c["w"], c["tol"], c["maxiter"], oracle, ref_errs=c["ref_errs"])
    return _PIN[c["key"]]


def check_count_and_pi(c, p, it, pi, oracle, what, r=None):
    """The rule of the module docstring; `r`: the fp32 losses the oracle's pi is taken on (default the case's)."""
    r = c["r"] if r is None else r
    if p["pinned"]:
        assert it == c["ref_iters"], (what, c["key"], it, c["ref_iters"])
        ref = p["pi"]
    else:
        assert it in p["feasible"] | {p["it32"], p["c64"]}, (what, c["key"], it, sorted(p["feasible"]))
        rr, ref = r.copy(), c["w"].copy()
        oracle.update_sample_weights(rr, ref, tol=0.0, maxiter=it)
    rel, small = rel_pi(pi, ref)
    assert rel <= REL and small <= 1e-7, (what, c["key"], it, rel, small)


def run_estep(torch, ops, dev, r, w, tol, maxiter, ws, trace=False):
    rt, wt = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(w.copy()).to(dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    tr = torch.zeros(2 * maxiter, device=dev) if trace else None
    ops.estep_deep(rt, wt, tol=tol, maxiter=maxiter, iters=iters, trace=tr, ws=ws)
    torch.cuda.synchronize()
    assert ws.status() == 0
    return int(iters), wt.cpu().numpy(), (tr.cpu().numpy()[0::2] if trace else None)


def drifted(r, scale, seed):
    rng = np.random.default_rng(seed)
    noise = (1.0 + 1e-3 * (scale - 1.0) * rng.standard_normal(r.shape[0]))
    return (r.astype(np.float64) * scale * noise).astype(np.float32)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("entry", entries())
def test_near_tie_estep_deep_every_path(entry, gpu, oracle):
    """One launch of estep_deep per path, on every case of the entry: a fresh workspace, the cold_start
    option, a warm start on the same vector, warm starts from drifted copies (0.1 %, 1 %, 5 %, 30 % and
    noise: how far off the first round's nodes are, and with it which accept path runs) with and without the
    verification round forced (RLVI_TJ_VERIFY=1), and a run with the error trace.  Accept and verify give
    the same count on pinned cases and pi within 4e-6 of each other.  With the trace, the step errors
    themselves: |err_kernel_j - err64_j| <= F tol for every test, F the largest per-test floor."""
    torch, ops, dev = gpu
    for key in cases_of(entry):
        c = g11_case(key)
        p = pin(c, oracle)
        r, w, tol, maxiter, N = c["r"], c["w"], c["tol"], c["maxiter"], c["N"]
        ws = ops.Workspace(dev, N, 0)
        it, pi, _ = run_estep(torch, ops, dev, r, w, tol, maxiter, ws)
        check_count_and_pi(c, p, it, pi, oracle, "fresh")
        it2, pi2, _ = run_estep(torch, ops, dev, r, w, tol, maxiter, ws)
        check_count_and_pi(c, p, it2, pi2, oracle, "warm, same vector")
        ws_c = ops.Workspace(dev, N, 0)
        ws_c.set_option("cold_start", 1)
        itc, pic, _ = run_estep(torch, ops, dev, r, w, tol, maxiter, ws_c)
        check_count_and_pi(c, p, itc, pic, oracle, "cold_start")
        for j, scale in enumerate(DRIFTS):
            rd = drifted(r, scale, 100 * entry + j)
            got = []
            for verify in (0, 1):
                tune("RLVI_TJ_VERIFY", verify)
                try:
                    wsd = ops.Workspace(dev, N, 0)
                    run_estep(torch, ops, dev, rd, np.ones(N, np.float32), tol, maxiter, wsd)    # warms the state
                    got.append(run_estep(torch, ops, dev, r, w, tol, maxiter, wsd))
                finally:
                    untune("RLVI_TJ_VERIFY")
            for verify, (itd, pid, _) in enumerate(got):
                check_count_and_pi(c, p, itd, pid, oracle, f"drift {scale} verify {verify}")
            if p["pinned"]:
                assert got[0][0] == got[1][0], (key, scale, got[0][0], got[1][0])
            if got[0][0] == got[1][0]:
                a, b = got[0][1].astype(np.float64), got[1][1].astype(np.float64)
                big = b >= 1e-6 * b.max()
                assert np.max(np.abs(a[big] - b[big]) / b[big]) <= 4e-6, (key, scale)
        itt, pit, errs = run_estep(torch, ops, dev, r, w, tol, maxiter, ops.Workspace(dev, N, 0), trace=True)
        check_count_and_pi(c, p, itt, pit, oracle, "trace")
        n = min(itt, p["c64"])
        F = float(p["floor"].max())
        dev_err = np.abs(errs[:n].astype(np.float64) - p["e64"][:n])
        assert np.all(dev_err <= F * tol), (key, int(np.argmax(dev_err - F * tol)), dev_err.max() / tol, F)


def _em_inputs(r, C):
    """Logits whose NLL is `r`: z_y = t, the other columns 0, CE = log1p((C-1) e^-t); the fp64 NLL of the fp32
    logits beside them."""
    B = r.shape[0]
    r64 = r.astype(np.float64)
    t = (np.log(C - 1.0) - np.log(np.expm1(np.maximum(r64, 1e-30)))).astype(np.float32)
    labels = (np.arange(B) * 7 % C).astype(np.int64)
    z = np.zeros((B, C), np.float32)
    z[np.arange(B), labels] = t
    t64 = t.astype(np.float64)
    nll64 = np.logaddexp(np.log(C - 1.0), t64) - t64
    return z, labels, nll64


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", [4096, 65536])
@pytest.mark.parametrize("C", [10, 100])
def test_near_tie_fused_em(B, C, gpu, oracle):
    """The in-batch E+M (the same solve inside fused_em, rlvi_trajb.h) on logits built to have the case's
    losses; the margins measured again from the fp64 NLL of the fp32 logits.  The same rule; the three-launch
    composition (RLVI_FUSED_EM=0) gives the same count on the pinned cases."""
    torch, ops, dev = gpu
    keys = [k for e in entries() for k in cases_of(e)
            if int(g11_meta(k)["N"]) == B and int(g11_meta(k)["maxiter"]) <= 64]
    assert keys
    for key in keys:
        c = g11_case(key)
        z, labels, nll64 = _em_inputs(c["r"], C)
        r32, _ = oracle.nll_rows(z, labels)
        p = pinning(r32, c["w"], c["tol"], c["maxiter"], oracle, r64=nll64)
        c = dict(c, ref_iters=p["it32"])          # (G11 holds the reference's count on the case's own losses)
        got = []
        for fused in (1, 0):
            tune("RLVI_FUSED_EM", fused)
            try:
                ws = ops.Workspace(dev, B, B)
                pit = torch.from_numpy(c["w"].copy()).to(dev)
                _, _, _, iters = ops.fused_em(torch.from_numpy(z).to(dev), torch.from_numpy(labels).to(dev), pit,
                                              tol=c["tol"], maxiter=c["maxiter"], ws=ws)
                torch.cuda.synchronize()
                assert ws.status() == 0
                got.append((int(iters), pit.cpu().numpy()))
            finally:
                untune("RLVI_FUSED_EM")
        for fused, (it, pi) in zip((1, 0), got):
            check_count_and_pi(c, p, it, pi, oracle, f"fused_em C={C} fused={fused}", r=r32)
        if p["pinned"]:
            assert got[0][0] == got[1][0], (key, C, got[0][0], got[1][0])


@pytest.mark.timeout(600)
def test_near_tie_epoch_end_with_truncation(gpu, oracle):
    """epoch_end (E-step + type-II threshold + truncation) on the pinned cases up to 262 144 samples: the
    reference's count, and threshold, truncated weights and kept count bit for bit the oracle's applied to the
    kernel's own pi (estep_deep on a fresh workspace: the same E-step launch)."""
    torch, ops, dev = gpu
    n_run = 0
    for key in g11_cases():
        meta = g11_meta(key)
        if meta["N"] > 262144:
            continue
        c = g11_case(key)
        p = pin(c, oracle)
        if not p["pinned"]:
            continue
        N = c["N"]
        _, pi_k, _ = run_estep(torch, ops, dev, c["r"], c["w"], c["tol"], c["maxiter"], ops.Workspace(dev, N, 0))
        ws = ops.Workspace(dev, N, 0)
        rt, wt = torch.from_numpy(c["r"].copy()).to(dev), torch.from_numpy(c["w"].copy()).to(dev)
        iters = torch.zeros(1, dtype=torch.int32, device=dev)
        thr, _ = ops.epoch_end(rt, wt, overfit=True, threshold=0.0, tol=c["tol"], maxiter=c["maxiter"],
                               iters=iters, ws=ws)
        torch.cuda.synchronize()
        assert ws.status() == 0
        assert int(iters) == c["ref_iters"], (key, int(iters), c["ref_iters"])
        t_o = oracle.false_negative_criterion(pi_k)
        w_o = pi_k.copy()
        m_o = oracle.truncate(w_o, t_o)
        wg = wt.cpu().numpy()
        assert float(thr) == float(t_o), key
        assert np.array_equal(wg, w_o), key
        n_run += 1
    assert n_run >= 100


def _sharded_near_tie_worker(rank, world, port, q, keys, sizes):
    import os as _os
    import sys as _sys
    here = _os.path.dirname(_os.path.abspath(__file__))
    _sys.path.insert(0, _os.path.dirname(here))
    _sys.path.insert(0, here)
    _os.environ["MASTER_ADDR"] = "127.0.0.1"
    _os.environ["MASTER_PORT"] = str(port)
    import torch as _torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rlvi_amd import _lib, ops as _ops
        from rlvi_amd import dist as rdist
        from test_near_ties_cpu import g11_case as _case
        dev = _torch.device("cuda:0")
        N = int(sum(sizes))
        ws = _ops.Workspace(dev, N, 0)
        peers = rdist.setup_peers(ws)
        assert rdist.declare_device_sharing() == world
        lo = int(sum(sizes[:rank]))
        hi = lo + int(sizes[rank])
        out = []
        for key in keys:
            c = _case(key)
            assert c["N"] == N
            can = [None] * world
            dist.all_gather_object(can, _lib.load().rlvi_estep_sharded_check(hi - lo, N, c["maxiter"], 0) == 0)
            assert all(can), can
            res = _torch.from_numpy(c["r"][lo:hi].copy()).to(dev)
            w = _torch.from_numpy(c["w"][lo:hi].copy()).to(dev)
            iters = _torch.zeros(1, dtype=_torch.int32, device=dev)
            dist.barrier()
            _ops.estep_sharded(res, w, N, tol=c["tol"], maxiter=c["maxiter"], iters=iters, ws=ws)
            _torch.cuda.synchronize()
            out.append((int(iters), w.cpu().numpy(), ws.status()))
        dist.barrier()
        peers.close()
        q.put((rank, "ok", out))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL " + repr(e) + "\n" + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("N", [4096, 65536])
def test_near_tie_sharded_estep_two_ranks_on_one_gpu(N, gpu, oracle):
    """The sharded E-step, 2 ranks on cuda:0 with unequal shards (3/8 and 5/8): each rank runs its own rounds
    and sums the totals in rank order, so its rounding differs from the single launch.  On the pinned cases
    every rank gives the reference's count and its slice of the oracle's pi; on the others, the rule of the
    module docstring on the whole vector."""
    import socket
    import torch.multiprocessing as mp
    keys = [k for k in g11_cases() if g11_meta(k)["N"] == N and g11_meta(k)["maxiter"] <= 64]
    assert keys
    sizes = (N * 3 // 8, N - N * 3 // 8)
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_near_tie_worker, args=(r, world, port, q, keys, sizes))
             for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(30)
    assert all(r[1] == "ok" for r in results), [r[1] for r in results]
    for i, key in enumerate(keys):
        c = g11_case(key)
        p = pin(c, oracle)
        its = [results[r][2][i][0] for r in range(world)]
        assert all(results[r][2][i][2] == 0 for r in range(world)), key
        assert its[0] == its[1], (key, its)            # (the ranks share one decision)
        pi = np.concatenate([results[r][2][i][1] for r in range(world)])
        check_count_and_pi(c, p, its[0], pi, oracle, "sharded")
