"""The argument contract of the one-launch fp64 estimators' C entries (standard.hip, logreg.hip, robust_logreg.hip,
moments.hip, robust_linreg.hip, online_sgd.hip): which code a defective call gets, and which defect wins when a call has
two -- RLVI_E_NULL before RLVI_E_SHAPE before RLVI_E_LIMIT before RLVI_E_ALIGN.

EVERY CALL IN THIS FILE CARRIES AT LEAST ONE DEFECT.  The addresses are fake, and the file also runs on machines that
have a GPU: a call that passed all checks would launch a kernel on them.  The calls are therefore made by _call alone,
which refuses an argument list without a defect (and a "defect" that leaves its argument at the good value)."""
import ctypes
import math

import pytest

E_NULL, E_SHAPE, E_ALIGN, E_LIMIT = -1, -2, -3, -5          # include/rlvi_hip.h
MAXN, MAXBATCH = 4096, 1 << 20

_buf = (ctypes.c_char * 8192)()
P = (ctypes.addressof(_buf) + 255) & ~255                   # what every good pointer is: aligned on 256 bytes
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from rlvi_amd import _build, _lib
    _build.build()
    return _lib.load()


class Entry:
    """One C entry: its arguments in the header's order with a good value each, and its defects by kind."""

    def __init__(self, name, args, required, shape, limit, f64, i32=("info",), optional=()):
        self.name, self.args = name, args
        self.required = required                            # pointers that must not be NULL
        self.shape, self.limit = shape, limit               # lists of {argument: bad value}
        self.f64, self.i32 = f64, tuple(a for a in i32 if a in dict(args))
        self.optional = optional                            # pointers that may be NULL
        self.ws = "ws" in dict(args)

    def align(self):
        out = [{a: P + 4} for a in self.f64] + [{a: P + 2} for a in self.i32]
        return out + ([{"ws": P + 8}] if self.ws else [])


def _call(lib, e, *defects, setup=None):
    """e's entry with the good arguments, `setup` (changes that are no defect: another method, no test rows) and
    `defects` laid over them.  Refuses a call without a defect."""
    if not defects:
        raise AssertionError("a call without a defect would launch a kernel on fake addresses")
    good = dict(e.args)
    good.update(setup or {})
    vals = dict(good)
    for dfc in defects:
        if not dfc:
            raise AssertionError("an empty defect")
        for k, v in dfc.items():
            same = v is good[k] or (not isinstance(v, float) or not math.isnan(v)) and v == good[k]
            if same:
                raise AssertionError(f"{e.name}: {k} = {v!r} is the good value, not a defect")
            vals[k] = v
    from rlvi_amd import _lib
    assert len(e.args) == len(_lib.SIGNATURES[e.name][1]), e.name
    return getattr(lib, e.name)(*[vals[k] for k, _ in e.args])


def _with_batch(args):
    """The batch form's arguments: `batch` in front of n."""
    i = [k for k, _ in args].index("n")
    return args[:i] + [("batch", 3)] + args[i:]


ENTRIES = []


def _family(name, args, required, shape, limit, f64, batch=True, **kw):
    """The single entry `name`_f64 and, with batch, its _batch_f64 form: the same contract + the batch count's."""
    ENTRIES.append(Entry(name + "_f64", args, required, shape, limit, f64, **kw))
    if batch:
        ENTRIES.append(Entry(name + "_batch_f64", _with_batch(args), required, shape + [{"batch": 0}, {"batch": -1}],
                             limit + [{"batch": MAXBATCH + 1}], f64, **kw))


_TAIL = [("info", P), ("ws", P), ("stream", None)]
_N = [{"n": 0}, {"n": -1}]
_D = [{"d": 0}, {"d": -3}]
# ((1 - eps) n <= 1 for every n the entries take: rl_eps_ok is false)
_EPS = [{"eps": 0.0}, {"eps": 1.0}, {"eps": NAN}, {"eps": 1.0 - 1e-6}]

_family("rlvi_linear_regression",
        [("X", P), ("y", P), ("n", 40), ("d", 10), ("maxiter", 5), ("tol", 1e-6), ("estep_tol", 1e-6),
         ("estep_maxiter", 5), ("theta", P), ("weights", P)] + _TAIL,
        required=["X", "y", "theta", "weights", "info", "ws"],
        shape=_N + _D + [{"maxiter": -1}, {"estep_maxiter": -1}],
        limit=[{"n": MAXN + 1}, {"d": 32}],
        f64=["X", "y", "theta", "weights"])
_family("rlvi_logistic_regression",
        [("X", P), ("y", P), ("n", 40), ("d", 10), ("maxiter", 5), ("tol", 1e-6), ("estep_tol", 1e-6),
         ("estep_maxiter", 5), ("C", 100.0), ("theta", P), ("weights", P), ("losses", P)] + _TAIL,
        required=["X", "y", "theta", "weights", "info", "ws"],
        shape=_N + _D + [{"maxiter": -1}, {"estep_maxiter": -1}, {"C": 0.0}, {"C": -1.0}, {"C": NAN}],
        limit=[{"n": MAXN + 1}, {"d": 31}],
        f64=["X", "y", "theta", "weights", "losses"], optional=["losses"])
_family("rlvi_logistic_fit",
        [("X", P), ("y", P), ("w", P), ("n", 40), ("d", 10), ("C", 100.0), ("theta", P), ("losses", P)] + _TAIL,
        required=["X", "y", "w", "theta", "losses", "info", "ws"],
        shape=_N + _D + [{"C": 0.0}, {"C": NAN}],
        limit=[{"n": MAXN + 1}, {"d": 31}],
        f64=["X", "y", "w", "theta", "losses"], batch=False)
_family("rlvi_rrm_logistic_regression",
        [("X", P), ("y", P), ("n", 40), ("d", 10), ("eps", 0.1), ("maxiter", 5), ("tol", 1e-6), ("C", 100.0),
         ("theta", P), ("weights", P)] + _TAIL,
        required=["X", "y", "theta", "weights", "info", "ws"],
        shape=_N + _D + _EPS + [{"maxiter": -1}, {"C": 0.0}, {"C": NAN}],
        limit=[{"n": MAXN + 1}, {"d": 31}],
        f64=["X", "y", "theta", "weights"])
_family("rlvi_rrm_linear_regression",
        [("X", P), ("y", P), ("n", 40), ("d", 10), ("eps", 0.1), ("maxiter", 5), ("tol", 1e-6), ("theta", P),
         ("weights", P)] + _TAIL,
        required=["X", "y", "theta", "weights", "info", "ws"],
        shape=_N + _D + _EPS + [{"maxiter": -1}],
        limit=[{"n": MAXN + 1}, {"d": 32}],
        f64=["X", "y", "theta", "weights"])
_family("rlvi_huber_linear_regression",
        [("X", P), ("y", P), ("n", 40), ("d", 10), ("c", 1.345), ("sigma0", 1.0), ("maxiter", 5), ("theta", P),
         ("scale", P)] + _TAIL,
        required=["X", "y", "theta", "scale", "info", "ws"],
        shape=_N + _D + [{"maxiter": -1}, {"c": 0.0}, {"c": NAN}, {"sigma0": 0.0}, {"sigma0": NAN}],
        limit=[{"n": MAXN + 1}, {"d": 32}],
        f64=["X", "y", "theta", "scale"])

# the moments: n = 1, d > 8 and n d > 16384 are limits, not shapes
_MO_LIMIT = [{"n": 1}, {"n": MAXN + 1}, {"d": 9}, {"n": MAXN, "d": 8}, {"n": 2049, "d": 8}]
_MO_OUT = [("theta", P), ("weights", P)] + _TAIL
for _fit, _extra in (("mean", []), ("pca", [("theta_init", P)]), ("covariance", [])):
    _rl = [("sample", P), ("n", 17), ("d", 2)] + ([("n_eff", 12.0)] if _fit == "covariance" else [])
    _family("rlvi_robust_" + _fit,
            _rl + [("maxiter", 5), ("tol", 1e-6)] + _extra + [("estep_tol", 1e-6), ("estep_maxiter", 5)] + _MO_OUT,
            required=["sample", "theta", "weights", "info", "ws"],
            shape=_N + _D + [{"maxiter": -1}, {"estep_maxiter": -1}], limit=_MO_LIMIT,
            f64=["sample", "theta", "weights"] + [k for k, _ in _extra], optional=[k for k, _ in _extra])
    _family("rlvi_rrm_" + _fit,
            [("sample", P), ("n", 17), ("d", 2), ("eps", 0.1), ("maxiter", 5), ("tol", 1e-6)] + _extra + _MO_OUT,
            required=["sample", "theta", "weights", "info", "ws"],
            shape=_N + _D + [{"maxiter": -1}], limit=_MO_LIMIT,
            f64=["sample", "theta", "weights"] + [k for k, _ in _extra], optional=[k for k, _ in _extra])

_family("rlvi_update_weights_constrained",
        [("losses", P), ("n", 40), ("n_eff", 30.0), ("tol", 1e-6), ("maxiter", 5), ("out", P)] + _TAIL,
        required=["losses", "out", "info", "ws"], shape=_N + [{"maxiter": -1}], limit=[{"n": MAXN + 1}],
        f64=["losses", "out"], batch=False)
_family("rlvi_rrm_update_weights",
        [("losses", P), ("n", 40), ("eps", 0.1), ("out", P)] + _TAIL,
        required=["losses", "out", "info", "ws"], shape=_N, limit=[{"n": MAXN + 1}],
        f64=["losses", "out"], batch=False)

# the online entries have no workspace; X and w of the weights entry are required unless `first`
_family("rlvi_sample_weight_online",
        [("X", P), ("w", P), ("b", 0.5), ("first", 0), ("n", 40), ("d", 10), ("tol", 1e-6), ("maxiter", 5),
         ("losses_out", P), ("sample_weight", P), ("out_iters", P), ("stream", None)],
        required=["X", "w", "sample_weight"], shape=_N + _D + [{"maxiter": -1}], limit=[{"n": MAXN + 1}],
        f64=["X", "w", "sample_weight", "losses_out"], i32=(), optional=["losses_out", "out_iters"], batch=False)
_family("rlvi_online_step",
        [("X", P), ("y", P), ("order", P), ("n", 40), ("d", 10), ("method", 3), ("eps", 0.1), ("first", 0),
         ("state", P), ("Xt", P), ("yt", P), ("m", 7), ("alpha", 1e-4), ("tol", 1e-6), ("maxiter", 5),
         ("sample_weight", P), ("counts", P), ("info", P), ("stream", None)],
        required=["X", "y", "state", "counts", "info", "Xt", "yt", "sample_weight"],      # (m > 0 and method 3)
        shape=_N + _D + [{"m": -1}, {"maxiter": -1}, {"method": -1}, {"method": 4}, {"alpha": 0.0}, {"alpha": NAN},
                         {"method": 2, "eps": 0.0}, {"method": 2, "eps": 1.0}, {"method": 2, "eps": NAN}],
        limit=[{"n": MAXN + 1}, {"m": MAXN + 1}, {"d": 129}],
        f64=["X", "y", "state", "Xt", "yt", "sample_weight"], i32=("order", "counts", "info"), optional=["order"],
        batch=False)

# online_stream reads `methods` and `eps` on the host: real arrays.  Classifier 1 is RRM, classifier 2 takes weights.
_METHODS = (ctypes.c_int32 * 3)(1, 2, 3)
_EPS3 = (ctypes.c_double * 3)(0.0, 0.1, 0.0)
_family("rlvi_online_stream",
        [("X", P), ("y", P), ("Xt", P), ("yt", P), ("rows", P), ("orders", P), ("T", 4), ("n", 40), ("m", 7), ("d", 10),
         ("methods", _METHODS), ("eps", _EPS3), ("S", 3), ("alpha", 1e-4), ("tol", 1e-6), ("maxiter", 5),
         ("state_hist", P), ("counts", P), ("weights", P), ("info", P), ("stream", None)],
        # (`weights` for method 3, `eps` and the values of both arrays: test_online_stream_per_classifier_checks)
        required=["X", "y", "methods", "state_hist", "counts", "info", "Xt", "yt"],
        shape=_N + _D + [{"T": 0}, {"S": 0}, {"m": -1}, {"maxiter": -1}, {"alpha": 0.0}, {"alpha": NAN}],
        limit=[{"n": MAXN + 1}, {"m": MAXN + 1}, {"d": 129}, {"S": 9}, {"T": (1 << 20) + 1}],
        f64=["X", "y", "Xt", "yt", "state_hist", "weights"], i32=("rows", "orders", "counts", "info"),
        optional=["rows", "orders"], batch=False)

BY_NAME = {e.name: e for e in ENTRIES}
NAMES = sorted(BY_NAME)


def test_every_launching_entry_of_the_six_files_is_covered():
    from rlvi_amd import _lib
    assert len(ENTRIES) == len(BY_NAME) == 28
    for e in ENTRIES:
        assert e.name in _lib.SIGNATURES
        assert e.shape and e.limit and e.required and e.align()


@pytest.mark.parametrize("name", NAMES)
def test_each_required_pointer_null(lib, name):
    e = BY_NAME[name]
    for a in e.required:
        assert _call(lib, e, {a: None}) == E_NULL, a


@pytest.mark.parametrize("name", NAMES)
def test_each_shape_defect(lib, name):
    e = BY_NAME[name]
    for dfc in e.shape:
        assert _call(lib, e, dfc) == E_SHAPE, dfc


@pytest.mark.parametrize("name", NAMES)
def test_each_limit_defect(lib, name):
    e = BY_NAME[name]
    for dfc in e.limit:
        assert _call(lib, e, dfc) == E_LIMIT, dfc


@pytest.mark.parametrize("name", NAMES)
def test_each_misaligned_address(lib, name):
    """fp64 arrays on 8 bytes, int32 arrays (info among them) on 4, the workspace on 256."""
    e = BY_NAME[name]
    for dfc in e.align():
        assert _call(lib, e, dfc) == E_ALIGN, dfc


@pytest.mark.parametrize("name", NAMES)
def test_precedence_of_adjacent_checks(lib, name):
    e = BY_NAME[name]
    for null in ({a: None} for a in e.required):
        assert _call(lib, e, null, e.shape[0]) == E_NULL
    pairs = 0
    for shape in e.shape:
        for limit in e.limit:
            if not set(limit) & set(shape):                 # (the two defects on different arguments)
                assert _call(lib, e, shape, limit) == E_SHAPE, (shape, limit)
                pairs += 1
    # (rrm_update_weights has n alone to be wrong in either way)
    assert pairs > 0 or name == "rlvi_rrm_update_weights_f64"
    for limit in e.limit:
        for al in e.align():
            assert _call(lib, e, limit, al) == E_LIMIT, (limit, al)


@pytest.mark.parametrize("name", NAMES)
def test_an_optional_pointer_may_be_null(lib, name):
    """NULL in an optional argument is neither RLVI_E_NULL nor RLVI_E_ALIGN: the call's other defect is reported."""
    e = BY_NAME[name]
    for a in e.optional:
        assert _call(lib, e, {a: None}, e.shape[0]) == E_SHAPE, a
        assert _call(lib, e, {a: None}, e.limit[0]) == E_LIMIT, a
        assert _call(lib, e, {a: None}, next(al for al in e.align() if a not in al)) == E_ALIGN, a


def test_check_entries():
    from rlvi_amd import _build, _lib
    _build.build()
    L = _lib.load()
    for f, dmax in ((L.rlvi_linear_regression_check, 31), (L.rlvi_logistic_regression_check, 30)):
        assert f(0, 3) == E_SHAPE and f(3, 0) == E_SHAPE and f(-1, 40) == E_SHAPE
        assert f(MAXN + 1, 3) == E_LIMIT and f(40, dmax + 1) == E_LIMIT
        assert f(MAXN, dmax) == 0 and f(1, 1) == 0
    f = L.rlvi_moments_check
    assert f(0, 3) == E_SHAPE and f(3, 0) == E_SHAPE
    assert f(1, 2) == E_LIMIT and f(17, 9) == E_LIMIT and f(2049, 8) == E_LIMIT and f(MAXN + 1, 1) == E_LIMIT
    assert f(2, 1) == 0 and f(2048, 8) == 0 and f(MAXN, 4) == 0


def test_sample_weight_online_needs_x_and_w_unless_first(lib):
    e = BY_NAME["rlvi_sample_weight_online_f64"]
    first = {"first": 1, "X": None, "w": None}
    assert _call(lib, e, {"n": 0}, setup=first) == E_SHAPE
    assert _call(lib, e, {"n": MAXN + 1}, setup=first) == E_LIMIT
    assert _call(lib, e, {"sample_weight": None}, setup=first) == E_NULL
    assert _call(lib, e, {"X": P + 4}, setup=first) == E_ALIGN              # (an address that is given is checked)


def test_online_step_conditional_pointers(lib):
    e = BY_NAME["rlvi_online_step_f64"]
    no_rows = {"m": 0, "Xt": None, "yt": None}                              # no test rows: Xt, yt not needed
    assert _call(lib, e, {"n": 0}, setup=no_rows) == E_SHAPE
    assert _call(lib, e, {"d": 129}, setup=no_rows) == E_LIMIT
    for me in (0, 1, 2):                                                    # the weights pointer: method 3 only
        assert _call(lib, e, {"n": 0}, setup={"method": me, "sample_weight": None}) == E_SHAPE
        assert _call(lib, e, {"X": P + 4}, setup={"method": me, "sample_weight": None}) == E_ALIGN
    assert _call(lib, e, {"n": MAXN + 1}, setup={"method": 1, "eps": 7.0}) == E_LIMIT     # eps: method 2 only


def test_online_stream_per_classifier_checks(lib):
    """The methods' checks run after the limits and before the alignment, and return their own codes."""
    e = BY_NAME["rlvi_online_stream_f64"]
    bad_method = {"methods": (ctypes.c_int32 * 3)(1, 5, 3)}
    bad_eps = {"eps": (ctypes.c_double * 3)(0.0, 1.5, 0.0)}
    no_rrm = {"methods": (ctypes.c_int32 * 3)(1, 1, 3)}
    no_given = {"methods": (ctypes.c_int32 * 3)(1, 2, 0)}
    assert _call(lib, e, {"weights": None}) == E_NULL                       # method 3 without weights
    assert _call(lib, e, {"eps": None}) == E_NULL                           # method 2 without an eps array
    assert _call(lib, e, {"X": P + 4}, setup=dict(no_rrm, eps=None)) == E_ALIGN         # no method 2: eps is optional
    assert _call(lib, e, {"X": P + 4}, setup=dict(no_given, weights=None)) == E_ALIGN
    assert _call(lib, e, bad_method) == E_SHAPE and _call(lib, e, bad_eps) == E_SHAPE
    assert _call(lib, e, {"eps": (ctypes.c_double * 3)(0.0, NAN, 0.0)}) == E_SHAPE
    assert _call(lib, e, {"methods": (ctypes.c_int32 * 3)(1, -1, 3)}) == E_SHAPE
    for dfc in (bad_method, bad_eps, {"weights": None}, {"eps": None}):
        assert _call(lib, e, dfc, {"n": MAXN + 1}) == E_LIMIT               # after the limits
        assert _call(lib, e, dfc, {"S": 9}) == E_LIMIT
    assert _call(lib, e, bad_method, {"X": P + 4}) == E_SHAPE               # before the alignment
    assert _call(lib, e, bad_eps, {"info": P + 2}) == E_SHAPE
    assert _call(lib, e, {"weights": None}, {"X": P + 4}) == E_NULL
    # the classifiers in order: the first defective one decides
    assert _call(lib, e, {"methods": (ctypes.c_int32 * 3)(9, 2, 3)}, {"weights": None}) == E_SHAPE
    assert _call(lib, e, {"methods": (ctypes.c_int32 * 3)(3, 9, 3)}, {"weights": None}) == E_NULL
    assert _call(lib, e, {"T": 0}, setup={"m": 0, "Xt": None, "yt": None}) == E_SHAPE


def test_the_helper_refuses_a_call_without_a_defect(lib):
    e = BY_NAME["rlvi_linear_regression_f64"]
    with pytest.raises(AssertionError):
        _call(lib, e)
    with pytest.raises(AssertionError):
        _call(lib, e, {})
    with pytest.raises(AssertionError):
        _call(lib, e, {"n": 40})                            # the good value
    with pytest.raises(AssertionError):
        _call(lib, e, {"X": P})
