"""Shared cases and the float64 reference of the kernel-machine tests (tests/test_svm.py on the CPU,
tests/test_svm_gpu.py on the device).

``svm_reference`` evaluates the attributes an SVMClassifier / SVMRegressor node carries (float32,
as the file stores them) in float64 numpy with direct differences; it shares no code with the C++
executor or the device kernel. The scikit-learn estimators are fitted on data that is exactly
float32-representable (a StandardScaler is applied in float32 arithmetic, as the Scaler node does),
so their support vectors export without rounding.

Tolerances, none of them taken from the code under test:

* executor against ``svm_reference`` (``dec_tol``): the executor accumulates in double and rounds
  once, so |dec - ref| <= one float32 rounding of ref (2^-24 |ref|) plus the double accumulation's
  own error, bounded by 2^-40 (sum |coef_i K_i| + |rho|). Outputs behind a float32 sigmoid / Platt
  stage (``out_tol``): that error carried through the stage (evaluated on the reference at
  dec +- dec_tol) plus 4 ulps of the larger of the row's outputs (exp, add, divide, and 1 - p).
* ``svm_reference`` against scikit-learn (``SKLEARN_TOL``): the gap comes from rounding dual_coef,
  rho and gamma to float32. Measured on the CPU against scikit-learn's float64 decision values over
  ``sk_inputs`` for the six ``SK_CASES``, largest |difference| (and the same over sum |coef|):
  svc_rbf / svc_platt 6.5e-8 (2.6e-10), ocsvm_rbf 7.9e-7 (9.8e-9), svr_poly 2.6e-7 (6.7e-9),
  svc_sigmoid 5.6e-8 (2.1e-10), svc_linear 8.2e-8 (7.6e-9). With a x4 margin on the largest ratio:
  SKLEARN_TOL = 4e-8 sum |coef|.
* device against ``svm_reference`` on the real-valued models (``device_tol``): the device's
  expansion form evaluated in float32 numpy (``expansion_f32``) on the test inputs, its largest
  deviation from float64, x4 (float32 summation order differs between numpy and the kernel). The
  deviations over ``sk_inputs``: svc_rbf / svc_platt 5.5e-6 (S = 318, sum |coef| = 250), ocsvm_rbf
  3.3e-6 (S = 100, 80), svr_poly 2.4e-6 (S = 321, 39), svc_sigmoid 4.3e-7 (S = 276, 268), svc_linear
  1.5e-6 (S = 232, 11); x4 that is at most 2.2e-5 on decision values that span 3.1 .. 7.1, below
  1e-4 of the range, which the tests assert.
* device on small integers (``exact_tol``): LINEAR and POLY are bit-equal to float64 (every
  product and partial sum is an integer below 2^24, asserted on the reference). RBF / SIGMOID reach
  expf / tanhf with an exact argument; the bound is FN_ULPS = 2 ulps of the function (the HIP math
  documentation lists 1 for both) plus one rounding per addition of a row's sum - ceil(S / 64)
  chained fmas, 4 butterfly steps, 2 block additions, rho - all relative to sum |coef_i K_i| + |rho|.
"""
import functools

import numpy as np

EPS = 2.0 ** -24          # half an ulp of 1: one float32 rounding
ULP = 2.0 ** -23
FN_ULPS = 2
SKLEARN_TOL = 4e-8        # x sum |coef| (the docstring above)
N_FEAT = 30

KERNELS = ("LINEAR", "POLY", "RBF", "SIGMOID")
ROWS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
FEATS = (1, 3, 4, 5, 15, 16, 17, 30, 64, 128, 256)   # 256: the device cap (plan.SVM_MAX_F)
SVS = (1, 15, 16, 17, 63, 64, 65, 130)


def shape_cases(kernel: str):
    """(rows, F, S) triples for one kernel type: every value of ROWS, FEATS and SVS appears, the
    three lists rotated against each other by a kernel-dependent step."""
    k = KERNELS.index(kernel)
    out = [(ROWS[i], FEATS[(i + 3 * k) % len(FEATS)], SVS[(i + k) % len(SVS)]) for i in range(len(ROWS))]
    assert {c[0] for c in out} == set(ROWS) and {c[1] for c in out} == set(FEATS) and {c[2] for c in out} == set(SVS)
    return out


def load(m):
    from igaming_platform_amd.native import native
    return native().OnnxModel.from_bytes(m.SerializeToString())


def node_attrs(om, ops=("SVMClassifier", "SVMRegressor")):
    """(op type, attributes) of the model's kernel-machine node, as the reader returns them."""
    n = next(n for n in om.nodes() if n["op_type"] in ops)
    return n["op_type"], dict(n["attrs"])


def scaler_attrs(om):
    n = next((n for n in om.nodes() if n["op_type"] == "Scaler"), None)
    return None if n is None else dict(n["attrs"])


def apply_scaler(sa, X):
    """The Scaler node in float32 arithmetic, as the executor runs it."""
    X = np.asarray(X, np.float32)
    if sa is None:
        return X
    return (X - np.asarray(sa["offset"], np.float32)) * np.asarray(sa["scale"], np.float32)


def kernel_matrix(a, X):
    """K(x, s) [N, S] in float64 with direct differences, and the [S, F] support vectors."""
    g, c0, deg = (float(v) for v in np.asarray(a["kernel_params"], np.float64)[:3])
    sv = np.asarray(a["support_vectors"], np.float64)
    S = int(a["n_supports"]) if "n_supports" in a else int(np.sum(a["vectors_per_class"]))
    sv = sv.reshape(S, -1)
    X = np.asarray(X, np.float64)
    kt = a.get("kernel_type", "LINEAR")
    if kt == "RBF":
        d2 = ((X[:, None, :] - sv[None, :, :]) ** 2).sum(axis=2)
        return np.exp(-g * d2), sv
    d = (X[:, None, :] * sv[None, :, :]).sum(axis=2)
    if kt == "LINEAR":
        return d, sv
    if kt == "POLY":
        return (g * d + c0) ** deg, sv
    assert kt == "SIGMOID"
    return np.tanh(g * d + c0), sv


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def stage(op, a, dec):
    """The operator's outputs for decision values ``dec`` (float64): regressor [N, 1]; classifier
    scores [N, 2] = [dec, -dec] through the post transform, or [p0, 1 - p0] with Platt scaling."""
    post = a.get("post_transform", "NONE")
    assert post in ("NONE", "LOGISTIC")
    f = _sig if post == "LOGISTIC" else (lambda z: z)
    if op == "SVMRegressor":
        v = np.where(dec > 0, 1.0, -1.0) if int(a.get("one_class", 0)) else dec
        return f(v)[:, None]
    if "prob_a" in a:
        p0 = 1.0 / (1.0 + np.exp(float(a["prob_a"][0]) * dec + float(a["prob_b"][0])))
        return np.stack([p0, 1.0 - p0], axis=1)
    return np.stack([f(dec), f(-dec)], axis=1)


def svm_reference(op, a, X):
    """dict(dec, mag, out, label) in float64: mag = sum |coef_i K_i| + |rho| (the scale of every
    rounding bound), label = the classifier's (classlabels[0] when dec > 0, with Platt the larger
    probability; None for a regressor)."""
    Km, _ = kernel_matrix(a, X)
    coef = np.asarray(a["coefficients"], np.float64)
    rho = float(np.asarray(a["rho"], np.float64)[0])
    dec = Km @ coef + rho
    mag = np.abs(Km) @ np.abs(coef) + abs(rho)
    out = stage(op, a, dec)
    label = None
    if op == "SVMClassifier":
        cl = np.asarray(a.get("classlabels_ints", [0, 1]))
        label = cl[(out[:, 1] > out[:, 0]).astype(int)] if "prob_a" in a else cl[(~(dec > 0)).astype(int)]
    return dict(dec=dec, mag=mag, out=out, label=label)


def dec_tol(ref):
    """Executor against the reference on dec: one float32 rounding of a double accumulation."""
    return EPS * np.abs(ref["dec"]) + 2.0 ** -40 * ref["mag"]


def out_tol(op, a, ref, tol):
    """A decision-value error ``tol`` carried through the output stage (on the reference), plus 4
    ulps of the row's largest output for the stage's own float32 arithmetic."""
    lo, hi = stage(op, a, ref["dec"] - tol), stage(op, a, ref["dec"] + tol)
    prop = np.maximum(np.abs(lo - ref["out"]), np.abs(hi - ref["out"]))
    return prop + 4 * ULP * np.abs(ref["out"]).max(axis=1, keepdims=True)


# ------------------------------------------------------------------------------ scikit-learn models
def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def sk_data():
    """Training data [400, 30] with unscaled columns (mean up to 50, spread 0.5 .. 8), float32-exact,
    its StandardScaler, the scaled data as the Scaler node computes it (float32) and two targets."""
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(42)
    mu, sd = rng.uniform(-50, 50, N_FEAT), rng.uniform(0.5, 8, N_FEAT)
    X = _f32(rng.standard_normal((400, N_FEAT)) * sd + mu)
    sc = StandardScaler().fit(X)
    off, scale = sc.mean_.astype(np.float32), (1.0 / sc.scale_).astype(np.float32)
    Xs = ((X.astype(np.float32) - off) * scale).astype(np.float64)
    y = (Xs[:, 0] + Xs[:, 1] * Xs[:, 2] + 0.5 * rng.standard_normal(400) > 0.3).astype(int)
    t = Xs[:, 3] - 0.5 * Xs[:, 4] ** 2 + 0.1 * rng.standard_normal(400)
    return X, sc, Xs, y, t


def sk_inputs(n=129, seed=9):
    """Unscaled test rows from the training distribution (float32)."""
    X = sk_data()[0]
    rng = np.random.default_rng(seed)
    return (X[rng.integers(0, len(X), n)] + rng.standard_normal((n, N_FEAT)) * 0.3).astype(np.float32)


SK_CASES = ("svc_rbf", "svc_platt", "ocsvm_rbf", "svr_poly", "svc_sigmoid", "svc_linear")


@functools.lru_cache(maxsize=None)
def sk_case(name):
    """(fitted estimator, scaler, ONNX model) of one case; every estimator is fitted on the scaled data."""
    from sklearn.svm import SVC, SVR, OneClassSVM
    from igaming_platform_amd.onnx import convert
    X, sc, Xs, y, t = sk_data()
    if name == "svc_rbf":
        est = SVC(kernel="rbf", C=1.0, gamma="scale").fit(Xs, y)
    elif name == "svc_platt":
        est = SVC(kernel="rbf", C=1.0, gamma="scale", probability=True, random_state=0).fit(Xs, y)
    elif name == "ocsvm_rbf":
        est = OneClassSVM(kernel="rbf", nu=0.2, gamma="scale").fit(Xs)
    elif name == "svr_poly":
        est = SVR(kernel="poly", degree=3, coef0=1.0, C=0.5).fit(Xs, t)
    elif name == "svc_sigmoid":
        est = SVC(kernel="sigmoid", coef0=0.0, gamma=0.01).fit(Xs, y)
    else:
        assert name == "svc_linear"
        est = SVC(kernel="linear", C=0.05).fit(Xs, y)
    return est, sc, convert.svm(est, N_FEAT, scaler=sc)


def sk_decision(est, Xs):
    """scikit-learn's float64 decision value in the operator's orientation (SVC: libsvm's, positive
    for classes_[0], i.e. minus decision_function; SVR: predict)."""
    name = type(est).__name__
    if name == "SVC":
        return -est.decision_function(Xs)
    return est.predict(Xs) if name == "SVR" else est.decision_function(Xs)


# ------------------------------------------------------------------------------ the device's form in float32
def expansion_f32(step, X):
    """dec as the device forms it, in float32 numpy on the host tables of ``plan.svm_tables``: the
    input affine as one fma (a float64 product-sum rounded once), float32 dot products, RBF by
    |x'|^2 + |s|^2 - 2 x'.s, float32 kernel function and sum."""
    from igaming_platform_amd.models.plan import svm_tables
    t = {k: (None if v is None else v.numpy()) for k, v in svm_tables(step).items()}
    F, S = step.in_dim, step.n_sv
    x = (np.asarray(X, np.float64) * t["scale"][:F].astype(np.float64) + t["shift"][:F]).astype(np.float32)
    sv, coef = t["sv"][:S, :F], t["coef"][:S]
    d = x @ sv.T
    g, c0 = np.float32(step.gamma), np.float32(step.coef0)
    if step.kernel == "RBF":
        xx = (x * x).sum(axis=1, dtype=np.float32)
        d2 = np.maximum((xx[:, None] + t["sv_norm"][None, :S]) - np.float32(2) * d, np.float32(0))
        Km = np.exp(-g * d2)
    elif step.kernel == "POLY":
        Km = (g * d + c0) ** np.float32(step.degree)
    elif step.kernel == "SIGMOID":
        Km = np.tanh(g * d + c0)
    else:
        Km = d
    assert Km.dtype == np.float32
    return (Km * coef[None, :]).sum(axis=1, dtype=np.float32) + np.float32(step.rho)


def device_tol(step, X, ref_dec):
    """x4 the largest deviation of ``expansion_f32`` from the float64 reference over ``X``."""
    return 4.0 * float(np.abs(expansion_f32(step, X).astype(np.float64) - ref_dec).max())


def bare(step):
    """The step without its output stage: its value is dec."""
    from dataclasses import replace
    return replace(step, platt=None, platt_flip=False, one_class=False, post_scale=1.0, post_shift=0.0, act="none")


def step_out(step, dec):
    """The step's output stage on decision values ``dec`` in float64 (SVMStep's order)."""
    v = np.asarray(dec, np.float64)
    if step.platt is not None:
        v = 1.0 / (1.0 + np.exp(step.platt[0] * v + step.platt[1]))
        if step.platt_flip:
            v = 1.0 - v
    if step.one_class:
        v = np.where(v > 0, 1.0, -1.0)
    v = v * step.post_scale + step.post_shift
    return _sig(v) if step.act == "sigmoid" else v


def step_out_tol(step, dec, tol):
    """As ``out_tol`` for a device step: the error ``tol`` on dec through the stage, plus 4 ulps of
    1 (every stage output, and the p that 1 - p is formed from, is at most 1) or of the output."""
    ref = step_out(step, dec)
    prop = np.maximum(np.abs(step_out(step, dec - tol) - ref), np.abs(step_out(step, dec + tol) - ref))
    return prop + 4 * ULP * np.maximum(np.abs(ref), 1.0 if (step.platt is not None or step.act == "sigmoid") else 0.0)


# ------------------------------------------------------------------------------ small-integer models
def exact_case(kernel, F, S, rows, seed=0, one_class=False):
    """A random small-integer model and inputs whose LINEAR / POLY values are exact in float32:
    support vectors in [-3, 3], coefficients in [-2, 2], inputs in [-1, 1] (wide models) or
    [-3, 3]; POLY degree 3 up to 17 columns, else 2, degree 1 when F = 1; gamma and coef0 integers
    for POLY, gamma a power of two for RBF (near 1 / (5 F): kernel values of order e^-1) and SIGMOID: an exact
    argument of expf / tanhf."""
    from igaming_platform_amd.onnx import builders
    deg = 1 if F == 1 else 3 if F <= 17 else 2
    kw = dict(LINEAR=dict(gamma=1.0, coef0=0.0), POLY=dict(gamma=1.0, coef0=1.0, degree=float(deg)),
              RBF=dict(gamma=2.0 ** -int(np.ceil(np.log2(5.0 * F)))), SIGMOID=dict(gamma=2.0 ** -5, coef0=0.25))[kernel]
    m = builders.build("svm", n_features=F, n_sv=S, kernel=kernel, integer=True, seed=seed, one_class=one_class, **kw)
    rng = np.random.default_rng(seed + 1000)
    r = 1 if F > 17 else 3
    X = rng.integers(-r, r + 1, (rows, F)).astype(np.float32)
    return m, X


def exact_tol(kernel, S, ref):
    """None for the bit-equal kernels (after asserting the integers stay below 2^24), else the
    bound of the module docstring."""
    if kernel in ("LINEAR", "POLY"):
        assert ref["mag"].max() < 2 ** 24
        return None
    n_round = -(-S // 64) + 4 + 2 + 1
    return (2 * FN_ULPS + n_round) * EPS * ref["mag"]
