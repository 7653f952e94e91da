"""The serial path of the trajectory E-step's first round (rlvi_trajb.h, rlvi_traj.h): the reducer of a node combines
its four gathering waves' partials with one quantity per lane, between the two hops of the exchange; behind it the
recurrence wave runs the fourth-order chain between two workgroup barriers that every other wave has to meet.

Scheduling only, so every case is held against the oracle and against itself: a sequence of calls through one fresh
workspace, per call status 0, the oracle's iteration count and pi within the suite's REL; then the whole sequence again
on another fresh workspace, bit for bit (a wrong partial in a total, or a wave that missed a barrier, shows up as a
wrong count, a hang, a timeout status or different bits).  The cases walk the branches around the combine and the
barriers: the accepting path at sizes from one sample per workgroup to one per thread, a number of exchanging
workgroups that leaves gathering waves with some or no records, the epoch end's reduction riding beside them, a stop
test inside the acceptance band (accept declined, the verification round runs), rounds without the fourth-order
chain, a NaN residual, and the in-batch kernels that share the solve.  The inputs' stop tests clear tol by 1e-4 in
the oracle's own trace, except where the case is the near tie itself (a golden G11 case, pinned by
tests/test_near_ties_cpu.py's rule).
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_estep_split_gpu import check_sequence, estep_call, gpu, knobs, ones, oracle_call, vec  # noqa: F401  (gpu: fixture)
from test_near_ties_cpu import g11_case, pinning
from test_oracle_golden import REL, rel_pi

pytestmark = pytest.mark.gpu

TOL = 1e-3
ST_NOCONV, ST_TIMEOUT = 4, 2


@pytest.mark.parametrize("N", [64, 4096, 16384, 65536])
def test_accepting_path_warm_on_the_same_vector(N, gpu, oracle):
    """A cold call, then three from the call before's trajectory on the same vector: the fourth-order first round
    through both barriers, accepted without a verification round.  64: one sample per exchanging workgroup;
    16 384: one sample per thread in 64 workgroups of full width; 65 536: the bench's geometry."""
    r = vec(N)
    check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 4)


def test_one_hundred_exchanging_workgroups(gpu, oracle):
    """RLVI_COOP_CAP = 100: the first gathering wave of a reducer has all its records, the second 36 of 64, the last
    two none -- the combine still adds their zeros (and +inf for the minimum) in wave order."""
    N = 16384
    r = vec(N, seed=6)
    with knobs(RLVI_COOP_CAP=100):
        check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3)


def _epoch(torch, ops, dev, ws, d, w_t, res_t, batches):
    N = d["logits"].shape[0]
    edges = np.linspace(0, N, batches + 1).astype(np.int64)
    for lo, hi in zip(edges[:-1], edges[1:]):
        rows = np.arange(lo, hi)
        ops.mstep_fwd_bwd(torch.from_numpy(d["logits"][rows]).to(dev), torch.from_numpy(d["labels"][rows]).to(dev),
                          torch.from_numpy(rows).to(dev), w_t, res_t, accumulate=True, ws=ws)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    _, out = ops.epoch_end(res_t, w_t, batches=batches, tol=TOL, iters=iters, ws=ws)
    torch.cuda.synchronize()
    st = ws.status()
    ws.clear_status()
    return st, int(iters), w_t.cpu().numpy(), out.cpu().numpy()


def test_epoch_end_with_pending_mstep_records(gpu, oracle):
    """Three epochs of accumulate-mode M-steps and ops.epoch_end through one workspace: workgroup G - 1 reduces the
    M-step records inside the solve; the second and third epoch's E-step starts from the epoch before's trajectory
    (the barriers of the fourth-order round beside the reduction)."""
    torch, ops, dev = gpu
    N, C, batches = 4096, 10, 3
    d = synth.mstep_inputs(N, C, N=N, seed=41)
    runs = []
    for rep in range(2):
        ws = ops.Workspace(dev, N, N)
        w_t, res_t = torch.ones(N, device=dev), torch.zeros(N, device=dev)
        runs.append([_epoch(torch, ops, dev, ws, d, w_t, res_t, batches) for _ in range(3)])
    w_o, res_o = ones(N), np.zeros(N, np.float32)
    edges = np.linspace(0, N, batches + 1).astype(np.int64)
    for e in range(3):
        refs = [oracle.mstep(d["logits"][lo:hi], d["labels"][lo:hi], np.arange(lo, hi), w_o, res_o)
                for lo, hi in zip(edges[:-1], edges[1:])]
        it_o, w_o, res_o = oracle_call(oracle, res_o, w_o)
        st, it, pi, out = runs[0][e]
        rel, small = rel_pi(pi, w_o)
        print(f"epoch {e}: status {st} iterations {it} (oracle {it_o}) pi rel {rel:.2e} small {small:.2e}")
        assert st == 0, (e, st)
        assert it == it_o, (e, it, it_o)
        assert rel <= REL and small <= 1e-7, (e, rel, small)
        assert float(out[0]) == pytest.approx(np.mean([float(x["loss"]) for x in refs]), rel=1e-5)
        assert float(out[1]) == pytest.approx(np.mean([float(x["prec1"]) for x in refs]), abs=1e-4)
        st2, it2, pi2, out2 = runs[1][e]
        assert st2 == 0 and it2 == it
        assert np.array_equal(pi2, pi) and np.array_equal(out2, out), f"epoch {e}: the repeat differs in bits"


@pytest.mark.parametrize("key", ["e14_bimodal_4096_k20_m1e-03_m", "e14_bimodal_4096_k20_m1e-03_p"])
def test_stop_test_inside_the_acceptance_band(key, gpu, oracle):
    """A golden near tie: stop test 20 sits 0.1 % under / over tol, inside the acceptance test's band (at least 1 %),
    so the warm first round passes its barriers, declines to accept and the verification round decides.  The
    case is pinned (the count is defined in fp32); the warm calls start from its own trajectory."""
    torch, ops, dev = gpu
    c = g11_case(key)
    assert c["tol"] == TOL
    p = pinning(c["r"], c["w"], c["tol"], 40, oracle, ref_errs=c["ref_errs"])
    assert p["pinned"] and p["it32"] == c["ref_iters"]
    N = c["N"]
    runs = []
    for rep in range(2):
        ws = ops.Workspace(dev, N, 0)
        runs.append([estep_call(gpu, ws, c["r"], c["w"]) for _ in range(3)])
    for i in range(3):
        st, it, pi, res = runs[0][i]
        rel, small = rel_pi(pi, p["pi"])
        print(f"call {i}: status {st} iterations {it} (reference {c['ref_iters']}) pi rel {rel:.2e} small {small:.2e}")
        assert st == 0, (i, st)
        assert it == c["ref_iters"], (i, it, c["ref_iters"])
        assert rel <= REL and small <= 1e-7, (i, rel, small)
        st2, it2, pi2, res2 = runs[1][i]
        assert st2 == 0 and it2 == it
        assert np.array_equal(pi2, pi) and np.array_equal(res2, res), f"call {i}: the repeat differs in bits"


@pytest.mark.parametrize("maxiter", [1, 2])
def test_maxiter_one_and_two(maxiter, gpu, oracle):
    """One node, two nodes: no pair, or one, for the acceptance test -- the helper wave runs on what there is and the
    barriers are met all the same."""
    N = 4096
    r = vec(N, seed=4)
    check_sequence(gpu, oracle, N, [(r, ones(N), {"maxiter": maxiter})] * 3)


def test_trace_between_warm_calls(gpu, oracle):
    """A requested trace takes the call off the fourth-order round (no barrier at all), the calls around it are on."""
    N = 4096
    r = vec(N, seed=3)
    check_sequence(gpu, oracle, N, [(r, ones(N), {}), (r, ones(N), {}), (r, ones(N), {"trace": True}),
                                    (r, ones(N), {})])


def test_cold_start_every_call(gpu, oracle):
    N = 4096
    r = vec(N, seed=2)
    check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3, options={"cold_start": 1})


def test_verification_round_forced(gpu, oracle):
    N = 4096
    r = vec(N, seed=5)
    with knobs(RLVI_TJ_VERIFY=1):
        check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3)


def test_one_nan_residual(gpu, oracle):
    """A NaN among the residuals of a warm call: the fourth-order round's sums are not finite (the round is not ok),
    every wave still meets the barriers, the solve ends with RLVI_ST_NOCONV -- not with a timeout -- and every
    weight is NaN, as the reference's min / mean over such a vector leave them.  The same on a cold call."""
    torch, ops, dev = gpu
    N = 4096
    r = vec(N, seed=8)
    bad = r.copy()
    bad[11] = np.nan
    for rep in range(2):
        ws = ops.Workspace(dev, N, 0)
        st, it, pi, _ = estep_call(gpu, ws, r, ones(N))
        assert st == 0
        for call in ("warm", "after the failed call"):
            st, it, pi, _ = estep_call(gpu, ws, bad, ones(N))
            print(f"{call}: status {st} iterations {it}")
            assert st & ST_TIMEOUT == 0, (call, st)
            assert st == ST_NOCONV, (call, st)
            assert np.isnan(pi).all(), call
        st, it, pi, _ = estep_call(gpu, ops.Workspace(dev, N, 0), bad, ones(N))
        assert st == ST_NOCONV and np.isnan(pi).all()
        # ... and the workspace is good for a clean call afterwards
        st, it, pi, _ = estep_call(gpu, ws, r, ones(N))
        it_o, pi_o, _ = oracle_call(oracle, r, ones(N))
        rel, small = rel_pi(pi, pi_o)
        assert st == 0 and it == it_o and rel <= REL and small <= 1e-7, (st, it, it_o, rel, small)


@pytest.mark.parametrize("B,C", [(4096, 10), (16384, 100)])
def test_fused_em_shares_the_solve(B, C, gpu, oracle):
    """The in-batch E+M kernels (the short-row 256-thread form and the 512-thread form whose spare waves only follow
    the barriers): three calls through one workspace, the second and third from the trajectory before; twice."""
    torch, ops, dev = gpu
    d = synth.mstep_inputs(B, C, seed=B + C)
    loss, _ = oracle.nll_rows(d["logits"], d["labels"])
    it_o, pi_o, _ = oracle_call(oracle, loss, ones(B))
    zt, yt = torch.from_numpy(d["logits"]).to(dev), torch.from_numpy(d["labels"]).to(dev)
    runs = []
    for rep in range(2):
        ws = ops.Workspace(dev, B, B)
        seq = []
        for call in range(3):
            pit = torch.ones(B, device=dev)
            out, grad, rows, iters = ops.fused_em(zt, yt, pit, tol=TOL, ws=ws)
            torch.cuda.synchronize()
            seq.append((ws.status(), int(iters), pit.cpu().numpy(), grad.cpu().numpy()))
            ws.clear_status()
        runs.append(seq)
    for call in range(3):
        st, it, pi, grad = runs[0][call]
        rel, small = rel_pi(pi, pi_o)
        print(f"call {call}: status {st} iterations {it} (oracle {it_o}) pi rel {rel:.2e} small {small:.2e}")
        assert st == 0, (call, st)
        assert it == it_o, (call, it, it_o)
        assert rel <= REL and small <= 1e-7, (call, rel, small)
        st2, it2, pi2, grad2 = runs[1][call]
        assert st2 == 0 and it2 == it
        assert np.array_equal(pi2, pi) and np.array_equal(grad2, grad), f"call {call}: the repeat differs in bits"
