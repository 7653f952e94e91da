"""The first round of the trajectory E-step with its acceptance test split over two waves (rlvi_traj.h:
tj_accept_guess on wave 1 beside the serial chain of wave 0, two workgroup barriers around it).

Every case is a sequence of calls on one fresh workspace that walks a branch around the two barriers: the
sizes from fewer samples than workgroups to four samples per thread, the warm call on the same vector (the
split path proper), the bench's drifting vectors, no guess at all, a requested trace, one to three nodes,
the forced verification round, fewer exchanging workgroups, and the in-batch E+M kernels that share the solve.
Per call: status 0, the oracle's iteration count, pi within the suite's REL.  Then the whole sequence again on
another fresh workspace: every call bit for bit what it was the first time (the split is scheduling only --
and a barrier that some wave missed shows up here as a hang, a timeout status or different bits).

The oracle's count is asked for without a tie exemption, so the inputs are seeds whose stop tests all clear
tol by 1e-4 relative in the oracle's own trace (asserted per call: a property of the input, not of the kernels).
"""
import numpy as np
import pytest

from rlvi_amd import synth
from test_oracle_golden import REL, rel_pi

pytestmark = pytest.mark.gpu

TOL = 1e-3
MARGIN = 1e-4          # every |err_k - tol| of the oracle's trace clears this, relative to tol


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rlvi_amd import _lib, ops
    _lib.load()
    return torch, ops, torch.device("cuda:0")


class knobs:
    """Process-wide tuning knobs for the length of a `with` block."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from rlvi_amd import _lib
        for k, v in self.kv.items():
            _lib.check(_lib.load().rlvi_tune_set(k.encode(), int(v)), "rlvi_tune_set")

    def __exit__(self, *exc):
        from rlvi_amd import _lib
        for k in self.kv:
            _lib.load().rlvi_tune_unset(k.encode())


def oracle_call(oracle, r, w, maxiter=40):
    """The oracle on copies: (iterations, pi, shifted residuals); the stop tests must not be near ties."""
    rr, ww = r.copy(), w.copy()
    it, err, _ = oracle.update_sample_weights(rr, ww, tol=TOL, maxiter=maxiter, trace=True)
    if len(err):
        margin = float(np.min(np.abs(err.astype(np.float64) - TOL))) / TOL
        assert margin >= MARGIN, f"ill-posed case: the oracle's stop test is a near tie ({margin:.2e})"
    return it, ww, rr


def estep_call(gpu, ws, r, w, maxiter=40, trace=False):
    torch, ops, dev = gpu
    rt, wt = torch.from_numpy(r.copy()).to(dev), torch.from_numpy(w.copy()).to(dev)
    iters = torch.zeros(1, dtype=torch.int32, device=dev)
    tr = torch.zeros(2 * maxiter, device=dev) if trace else None
    ops.estep_deep(rt, wt, tol=TOL, maxiter=maxiter, iters=iters, trace=tr, ws=ws)
    torch.cuda.synchronize()
    st = ws.status()
    ws.clear_status()
    return st, int(iters), wt.cpu().numpy(), rt.cpu().numpy()


def check_sequence(gpu, oracle, N, calls, options=None):
    """calls: [(residuals, caller's pi, keyword arguments of estep_call)].  Twice, each on a fresh workspace."""
    torch, ops, dev = gpu
    runs = []
    for rep in range(2):
        ws = ops.Workspace(dev, N, 0)
        for k, v in (options or {}).items():
            ws.set_option(k, v)
        runs.append([estep_call(gpu, ws, r, w, **kw) for r, w, kw in calls])
    for i, (r, w, kw) in enumerate(calls):
        st, it, pi, res = runs[0][i]
        it_o, pi_o, res_o = oracle_call(oracle, r, w, kw.get("maxiter", 40))
        print(f"call {i}: status {st} iterations {it} (oracle {it_o})", end=" ")
        assert st == 0, (i, st)
        assert it == it_o, (i, it, it_o)
        rel, small = rel_pi(pi, pi_o)
        print(f"pi rel {rel:.2e} small {small:.2e}")
        assert rel <= REL and small <= 1e-7, (i, rel, small)
        assert np.array_equal(res, res_o), i
        st2, it2, pi2, res2 = runs[1][i]
        assert st2 == 0 and it2 == it, (i, st2, it2, it)
        assert np.array_equal(pi2, pi) and np.array_equal(res2, res), f"call {i}: the repeat differs in bits"


def vec(N, kind="bimodal", seed=None):
    return synth.residual_vector(kind, N, seed=N if seed is None else seed)


def ones(N):
    return np.ones(N, np.float32)


SIZES = [(64, "bimodal"), (300, "bimodal"), (4096, "bimodal"), (54000, "bimodal"), (65536, "bimodal"),
         (65537, "bimodal"), (75750, "zeros10"), (131072, "bimodal"), (262144, "bimodal")]


@pytest.mark.parametrize("N,kind", SIZES)
def test_sizes_cold_then_warm(N, kind, gpu, oracle):
    """A first call without a guess (no fourth-order round, no new barriers), then two with the trajectory of
    the call before (the split first round); a random caller's pi on the last one."""
    r = vec(N, kind)
    w_rand = np.random.default_rng(N).random(N).astype(np.float32)
    check_sequence(gpu, oracle, N, [(r, ones(N), {}), (r, ones(N), {}), (r, w_rand, {})])


def test_warm_on_the_same_vector(gpu, oracle):
    """The bench's estep_us: the same vector call after call."""
    N = 65536
    r = vec(N, seed=1)
    check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 5)


def drift_vectors(N):
    """bench.py's estep_drift_us: the bimodal vector scaled by 1.02^k plus noise, k walking 0..4..0."""
    rng = np.random.default_rng(11)
    base = vec(N, seed=0)
    dr = [(base * np.float32(1.02 ** k) + np.float32(0.01) * rng.random(N).astype(np.float32)).astype(np.float32)
          for k in range(5)]
    return [dr[k] for k in [0, 1, 2, 3, 4, 3, 2, 1] * 2]


def test_drift_walk(gpu, oracle):
    """Every call's guess is a neighbour's trajectory: the split first round, accepted or followed by a
    verification round as its bands decide."""
    N = 65536
    check_sequence(gpu, oracle, N, [(r, ones(N), {}) for r in drift_vectors(N)])


def test_cold_start_option(gpu, oracle):
    """No guess, call after call: the first round goes to the global model and takes neither barrier."""
    N = 65536
    r = vec(N, seed=2)
    check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3, options={"cold_start": 1})


def test_trace_requested(gpu, oracle):
    """A requested error trace switches the fourth-order round off for that call only."""
    N = 65536
    r = vec(N, seed=3)
    check_sequence(gpu, oracle, N, [(r, ones(N), {}), (r, ones(N), {"trace": True}), (r, ones(N), {}),
                                    (r, ones(N), {"trace": True})])


@pytest.mark.parametrize("maxiter", [1, 2, 3])
def test_maxiter_one_two_three(maxiter, gpu, oracle):
    """One to three nodes: fewer than two steps leave no pair to test (the acceptance block is skipped, the
    barriers are not); the second and third call are warm."""
    N = 65536
    r = vec(N, seed=4)
    check_sequence(gpu, oracle, N, [(r, ones(N), {"maxiter": maxiter})] * 3)


def test_verification_round_forced(gpu, oracle):
    N = 65536
    r = vec(N, seed=5)
    with knobs(RLVI_TJ_VERIFY=1):
        check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3)


@pytest.mark.parametrize("cap", [64, 128])
def test_fewer_exchanging_workgroups(cap, gpu, oracle):
    """RLVI_COOP_CAP: 64 and 128 exchanging workgroups (four and two samples per thread at this size)."""
    N = 65536
    r = vec(N, seed=6)
    with knobs(RLVI_COOP_CAP=cap):
        check_sequence(gpu, oracle, N, [(r, ones(N), {})] * 3)


@pytest.mark.parametrize("B,C", [(65536, 100), (16384, 100), (4096, 10)])
def test_fused_em_shares_the_solve(B, C, gpu, oracle):
    """The in-batch E+M kernels call the same solve (512-thread workgroups whose second half only shares the
    sums and follows the barriers, and the 256-thread short-row forms): two calls through one workspace, the
    second from the first one's trajectory; then all of it again."""
    torch, ops, dev = gpu
    d = synth.mstep_inputs(B, C, seed=B + C)
    loss, _ = oracle.nll_rows(d["logits"], d["labels"])
    it_o, pi_o, rows_o = oracle_call(oracle, loss, ones(B))
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
