"""The premises of tests/test_linreg_designs_gpu.py, checked on the float64 restatement and the references alone
(tests/linreg_designs.py) before any kernel is involved: a power-of-two column scaling changes no bit of the normal
equations' solution, the pivot test against a column's OWN diagonal entry is free of scale and still names rank
deficiency, which patterns the rule before flagged, what a badly CONDITIONED design costs, and that the oracle's outer
counts on the scaled designs are decided away from tol.  Each test prints its figures before it asserts."""
import numpy as np
import pytest

import linreg_designs as L

ALL_SHAPES = L.SHAPES + [s for s in L.EXACT_SHAPES if s not in L.SHAPES]


def both_weights(n):
    return (("unit", np.ones(n)), ("weighted", L.weights(n)))


def test_exact_wls_is_the_truth():
    """a system with a rational solution that no float holds exactly, solved exactly; a well-conditioned design
    against lstsq; and the exact solution of a scaled design is the scaled exact solution"""
    X = np.array([[1.0, 0.0], [1.0, 1.0], [1.0, 2.0]])
    y = np.array([0.0, 1.0, 1.0])
    np.testing.assert_array_equal(L.exact_wls(X, y, np.ones(3)), np.array([1.0 / 6.0, 0.5]))
    X, y = L.base(40, 10)
    w = L.weights(40)
    sw = np.sqrt(w)
    ex = L.exact_wls(X, y, w)
    # (sqrt(w) is rounded: lstsq solves a problem 1 ulp away in every row)
    np.testing.assert_allclose(np.linalg.lstsq(sw[:, None] * X, sw * y, rcond=None)[0], ex, rtol=1e-13)
    name, kv = L.patterns(10)[-1]
    assert name == "graded"
    np.testing.assert_array_equal(L.unscale(L.exact_wls(L.scaled(X, kv), y, w), kv), ex)
    assert L.kappa_eq(L.scaled(X, kv), w) == pytest.approx(L.kappa_eq(X, w), rel=1e-12)


@pytest.mark.parametrize("n,d", ALL_SHAPES)
def test_restatement_is_invariant_under_power_of_two_scaling(n, d):
    """rule="own": restate_wls(scaled(X, k)) 2^k has the BITS of restate_wls(X), for every pattern -- |k| up to 200,
    every position, all columns graded -- with unit weights and with weights(n)"""
    X, y = L.base(n, d)
    for wname, w in both_weights(n):
        th0 = L.restate_wls(X, y, w, "own")
        assert th0 is not None
        for name, kv in L.patterns(d):
            th = L.restate_wls(L.scaled(X, kv), y, w, "own")
            assert th is not None, (wname, name)
            assert np.array_equal(L.unscale(th, kv), th0), (wname, name)


@pytest.mark.parametrize("n,d", ALL_SHAPES)
def test_what_the_rule_before_flagged(n, d):
    """rule="dmax" on the scaled design flags exactly what the UNSCALED factorisation predicts: the scaled design's
    pivots are 2^2k times the unscaled ones (the invariance above), so it is flagged when min_j 4^k_j piv_j <=
    max_j 4^k_j G_jj d 64 eps -- with piv_j <= G_jj, whenever the scale ratio squared is below d 64 eps times a factor
    of order one.  Which patterns those are is linreg_designs.old_rule_accepts, the record; and every design that rule
    accepts, the new one accepts with the same bits."""
    X, y = L.base(n, d)
    for wname, w in both_weights(n):
        diag, piv = L.pivots(X, w)
        accepted = []
        for name, kv in L.patterns(d):
            s2 = np.ldexp(1.0, 2 * kv)
            predicted = bool(np.min(s2 * piv) <= np.max(s2 * diag) * d * 64 * L.EPS)
            Xs = L.scaled(X, kv)
            old = L.restate_wls(Xs, y, w, "dmax")
            assert (old is None) == predicted, (wname, name)
            if d > 1 and L.scale_ratio_sq(kv) < d * 64 * L.EPS:
                assert old is None, (wname, name)
            if old is not None:
                accepted.append(name)
                assert np.array_equal(old, L.restate_wls(Xs, y, w, "own")), (wname, name)
        print(f"{n} x {d} {wname}: the rule before accepts {accepted}")
        assert accepted == L.old_rule_accepts(n, d), wname


@pytest.mark.parametrize("n,d", ALL_SHAPES)
def test_rank_deficient_designs_are_flagged_under_both_rules(n, d):
    """a duplicated column, a duplicate times 2^-23, an all-zero column -- and the same three with a column scaling on
    top under the scale-free rule"""
    X, y = L.base(n, d)
    for wname, w in both_weights(n):
        for case, Z in L.rank_deficient(X).items():
            for rule in ("dmax", "own"):
                assert L.restate_wls(Z, y, w, rule) is None, (wname, case, rule)
            for name, kv in L.patterns(d):
                assert L.restate_wls(L.scaled(Z, kv), y, w, "own") is None, (wname, case, name)


def test_ladder_is_accepted_and_loses_kappa_eq_squared():
    """columns 1e2 ... 1e4 from the origin, a last column within 1e-3 / 1e-5 of the first: accepted under both rules,
    with the same bits, and within 2 r kappa_eq^2 eps of the exact rational solution (r = R_MEASURED, measured on
    exactly these solves); the well-scaled base designs are printed beside them"""
    worst = 0.0
    for n, d in L.EXACT_SHAPES:
        for weighted in (False, True):
            for case in ("base",) + L.LADDER_CASES:
                X, y, w, exact, kq = L.exact_case(n, d, case, weighted)
                th = L.restate_wls(X, y, w, "own")
                old = L.restate_wls(X, y, w, "dmax")
                assert th is not None and old is not None and np.array_equal(th, old), (n, d, case, weighted)
                err = L.rel_err(th, exact)
                ratio = err / (kq * kq * L.EPS)
                print(f"{n} x {d} {case:14s} weighted {int(weighted)}: kappa_eq {kq:9.3g} error {err:9.3g} = "
                      f"{ratio:6.3f} kappa_eq^2 eps")
                if case != "base":
                    worst = max(worst, ratio)
                    assert ratio <= 2 * L.R_MEASURED, (n, d, case, weighted)
    print("largest ratio over the ladder:", worst, "(R_MEASURED", L.R_MEASURED, ", C_BAR", L.C_BAR, ")")
    assert worst <= L.R_MEASURED                    # the committed constant is what was measured, not less
    assert L.C_BAR == 8.0
    # the bar of the GPU tests at the ladder's worst conditioning still catches a wrong coefficient
    assert L.C_BAR * max(L.exact_case(n, d, c, wt)[4] for n, d in L.EXACT_SHAPES for c in L.LADDER_CASES
                         for wt in (False, True)) ** 2 * L.EPS < 1e-3


@pytest.mark.parametrize("n,d", L.SHAPES)
def test_outer_counts_are_clear_of_the_edge(n, d, oracle):
    """Every case the GPU test compares outer counts on -- EVERY pattern of oracle_patterns(d) at every shape, none
    left out: a shape whose seed n + d fails this gets another seed in linreg_designs.SEEDS -- has each discrepancy of
    the oracle's stop test at least 1 % away from tol: the oracle's lstsq is good to kappa eps = 1e-6 of the
    discrepancy on these designs, so its count is a reference only away from the edge.  oracle_trace is the oracle's
    own loop: same theta bits, same count."""
    X, y = L.base(n, d)
    for name, kv in L.oracle_patterns(d):
        Xs = L.scaled(X, kv)
        th, w, outer, discs = L.oracle_trace(oracle, Xs, y)
        th_o, w_o, outer_o = oracle.linear_regression(Xs, y, trace=True)
        assert outer == outer_o and np.array_equal(th, th_o) and np.array_equal(w, w_o)
        margin = min(abs(x - 1e-3) / 1e-3 for x in discs)
        print(f"{n} x {d} {name}: outer {outer}, nearest discrepancy {margin:.3f} tol away from tol")
        assert len(discs) == outer < 100 and margin >= L.OUTER_MARGIN, (name, discs)
        # the oracle on the scaled design against the scale-free restatement at the oracle's own final weights: within
        # half the 1e-6 at which the GPU test compares theta with it (gelsd's kappa eps: 1e-7 ... 1.3e-6 at 2^-30,
        # seed by seed)
        rs = L.restate_wls(X, y, w, "own")
        print(f"    oracle against the restatement: {np.max(np.abs(L.unscale(th, kv) - rs) / np.abs(rs)):.3g}")
        np.testing.assert_allclose(L.unscale(th, kv), rs, rtol=L.ORACLE_PREC, err_msg=name)
