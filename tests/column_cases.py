"""Shared cases of the column-operator tests (tests/test_columns.py on the CPU, tests/test_columns_gpu.py
on the device): numpy references of the operators, random column programs with their value probes,
and fitted scikit-learn ColumnTransformer pipelines.

References. Every operator is exact in float32 except the Scaler, whose definition *is* its float32
evaluation ``(x - offset) * scale`` (one f32 subtract, one f32 multiply): the executor and the device
kernel must both reproduce it bit for bit, so every comparison against these references is for
equality (NaN equal to NaN, -0.0 distinguished from 0.0 only where the operator passes values through).

* ``Imputer``        y = hit ? v_c : x; hit = isnan(x) for a NaN replaced value, else x == replaced.
* ``OneHotEncoder``  a float matches category c when it is finite, |x| < 2^63 and (int64)trunc(x) == c.
* ``Binarizer``      y = x > t ? 1 : 0 (NaN gives 0).
* ``eval_records``   a ColumnStep's program: x = X[:, src]; impute; (x - sub) * mul; mode.

Against scikit-learn's own ``ct.transform`` (float64) a scaled column may differ by rounding only:
|y - y_sk| <= 2^-23 (3 |y_sk| + |scale * offset|), the first-order bound for rounding offset and
scale to float32 plus the two float32 operations, doubled. The float32 evaluation reaches 0.314 of it
for StandardScaler and 0.338 for MinMaxScaler on the data below, imputed rows included."""
import functools

import numpy as np

from igaming_platform_amd.models.plan import ColRec

ULP = 2.0 ** -23
N_FEAT = 30
TWO63 = 2.0 ** 63


def load(m):
    from igaming_platform_amd.native import native
    return native().OnnxModel.from_bytes(m.SerializeToString())


def run(m, X, name="output"):
    from igaming_platform_amd.native import native
    X = np.asarray(X)
    if X.dtype != np.int64:
        X = X.astype(np.float32)
    return np.asarray(native().Executor(load(m)).run({"input": X})[name])


def same(a, b):
    """Bit-equal as float32 values (NaN equal to NaN; 0.0 equal to -0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


# ------------------------------------------------------------------------------ operator references
def ref_imputer(x, values, replaced=0.0):
    x = np.asarray(x, np.float32)
    v = np.broadcast_to(np.asarray(values, np.float32), x.shape[-1:])
    rep = np.float32(replaced)
    hit = np.isnan(x) if np.isnan(rep) else x == rep
    return np.where(hit, v, x).astype(np.float32)


def ref_scaler(x, offset, scale):
    return ((np.asarray(x, np.float32) - np.asarray(offset, np.float32)) * np.asarray(scale, np.float32)).astype(np.float32)


def ref_onehot(x, cats):
    """Input shape + [n_cats], float32; ``x`` float32 or int64."""
    x = np.asarray(x)
    cats = np.asarray(cats, np.int64)
    if x.dtype == np.int64:
        return (x[..., None] == cats).astype(np.float32)
    x64 = x.astype(np.float64)
    valid = np.isfinite(x64) & (np.abs(x64) < TWO63)
    xi = np.trunc(np.where(valid, x64, 0.0)).astype(np.int64)   # exact: an f32 integer inside int64
    return (valid[..., None] & (xi[..., None] == cats)).astype(np.float32)


def ref_binarizer(x, threshold=0.0):
    return (np.asarray(x, np.float32) > np.float32(threshold)).astype(np.float32)


def ref_cast_int64(x):
    """Cast float -> int64 as the executor defines it: truncation; NaN / out of range -> INT64_MIN."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    ok = (x64 >= -TWO63) & (x64 < TWO63)
    return np.where(ok, np.trunc(np.where(ok, x64, 0.0)).astype(np.int64), np.iinfo(np.int64).min)


def eval_records(records, X):
    """A column program on X [M, >= in_width] in float32, stage by stage as ColRec defines them."""
    X = np.asarray(X, np.float32)
    out = np.zeros((X.shape[0], len(records)), np.float32)
    for j, r in enumerate(records):
        x = X[:, r.src].copy()
        if r.imp is not None:
            x = ref_imputer(x[:, None], [r.imp[1]], r.imp[0])[:, 0]
        if r.aff is not None:
            with np.errstate(all="ignore"):
                x = ref_scaler(x, r.aff[0], r.aff[1])
        if r.mode == "onehot":
            x = ref_onehot(x, [int(r.arg)])[:, 0]
        elif r.mode == "binarize":
            x = ref_binarizer(x, r.arg)
        elif r.mode == "zero":
            x = np.zeros_like(x)
        out[:, j] = x
    return out


# ------------------------------------------------------------------------------ probes and random programs
CATS = (-3, -1, 0, 1, 2, 7, 2 ** 24 + 1)     # 2^24 + 1: no float32 equals it, so it never matches
THRESHOLD = 0.5
SENTINEL = -999.0


def probe_values():
    """Edge inputs: NaN, +-inf, +-0.0; every category c at c, c +- 0.5, nextafter(c, +-inf); -0.5 (matches
    category 0); +-2^63; the binariser's threshold and the next float above it; the -999 sentinel."""
    v = [np.nan, np.inf, -np.inf, 0.0, -0.0, -0.5, TWO63, -TWO63, THRESHOLD, SENTINEL,
         float(np.nextafter(np.float32(THRESHOLD), np.float32(np.inf))),
         float(np.nextafter(np.float32(THRESHOLD), np.float32(-np.inf)))]
    for c in CATS:
        f = np.float32(c)
        v += [float(f), float(f) + 0.5, float(f) - 0.5, float(np.nextafter(f, np.float32(np.inf))),
              float(np.nextafter(f, np.float32(-np.inf)))]
    return np.asarray(v, np.float32)


def probe_matrix(rows, width, seed=0):
    """[rows, width] float32: random values with the probes scattered over every column."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-4, 9, (rows, width)).astype(np.float32)
    X[rng.random((rows, width)) < 0.3] = np.float32(rng.integers(-3, 8))
    p = probe_values()
    mask = rng.random((rows, width)) < 0.5
    X[mask] = p[rng.integers(0, len(p), int(mask.sum()))]
    return X


def random_records(in_width, out_width, seed=0):
    """A program that uses every record stage in every combination the plan can produce; sources are
    drawn with replacement (some read many times, some never)."""
    rng = np.random.default_rng(seed)
    recs = []
    for j in range(out_width):
        src = int(rng.integers(0, in_width))
        imp = [None, (float("nan"), 0.25), (SENTINEL, 1.5), (0.0, -2.0)][int(rng.integers(0, 4))]
        aff = None if rng.random() < 0.4 else (float(np.float32(rng.uniform(-2, 2))), float(np.float32(rng.uniform(0.25, 3))))
        mode = ["pass", "onehot", "binarize", "zero"][int(rng.choice(4, p=[0.4, 0.35, 0.2, 0.05]))]
        arg = 0.0
        if mode == "onehot":
            c = CATS[int(rng.integers(0, len(CATS)))]
            if int(np.float32(c)) != c:
                mode = "zero"
            else:
                arg = float(c)
            if rng.random() < 0.6:
                aff = None   # most encoders read the raw value
        elif mode == "binarize":
            arg = THRESHOLD
        recs.append(ColRec(src, imp, aff, mode, arg))
    return recs


# ------------------------------------------------------------------------------ scikit-learn pipelines
NUM = slice(0, 10)                 # imputed (median) and standardised
AMT = [10, 11, 12]                 # -999 sentinel imputed (mean), min-max scaled
CAT = [13, 14, 15]                 # transaction type (8), country (193), device class (5): one-hot
FLAG = np.arange(N_FEAT) // 4 == 4  # a boolean mask: columns 16 .. 19, binarised at 0.5
PASS = [20, 21, 22, 23, 24, 25]    # passed through
GONE = [26, 27]                    # dropped; 28, 29 are the dropped remainder
N_CAT = (8, 193, 5)
OUT_WIDTH = 10 + 3 + sum(N_CAT) + 4 + 6     # 229


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _rows(n, rng, train):
    X = np.zeros((n, N_FEAT))
    X[:, NUM] = rng.standard_normal((n, 10)) * rng.uniform(0.5, 8, 10) + np.linspace(-50, 50, 10)
    X[:, AMT] = rng.gamma(2.0, 40.0, (n, 3))
    for k, c in zip(CAT, N_CAT):
        X[:, k] = rng.integers(0, c, n)
        if train:
            X[:c, k] = np.arange(c)    # every category is seen in training
    X[:, 16:20] = rng.random((n, 4))
    X[:, 20:] = rng.standard_normal((n, 10))
    X = _f32(X)
    X[:, 0:10][rng.random((n, 10)) < 0.1] = np.nan          # slices: views of X
    X[:, 10:13][rng.random((n, 3)) < 0.1] = SENTINEL
    return X


@functools.lru_cache(maxsize=None)
def sk_data():
    """(training rows [600, 30], labels, test rows [257, 30]): float32-exact values held in float64."""
    rng = np.random.default_rng(7)
    X = _rows(600, rng, True)
    z = (np.nan_to_num(X[:, 3], nan=0.0) / 8 + (X[:, 13] % 3 == 0) * 1.5 - (X[:, 17] > 0.5) + X[:, 21]
         + 0.5 * rng.standard_normal(600))
    Xt = _rows(257, np.random.default_rng(8), False)
    Xt[5, 13], Xt[6, 14] = 11.0, 500.0     # categories never seen: all-zero blocks
    return X, (z > np.median(z)).astype(np.int64), Xt


@functools.lru_cache(maxsize=None)
def sk_transformer():
    """The fitted ColumnTransformer with all five branch kinds (plus a MinMaxScaler one): 30 -> 229."""
    from sklearn.compose import ColumnTransformer
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import Binarizer, MinMaxScaler, OneHotEncoder, StandardScaler
    X, _, _ = sk_data()
    ct = ColumnTransformer([
        ("num", Pipeline([("imp", SimpleImputer(strategy="median")), ("std", StandardScaler())]), NUM),
        ("amt", Pipeline([("imp", SimpleImputer(missing_values=SENTINEL, strategy="mean")), ("mm", MinMaxScaler())]), AMT),
        ("cat", OneHotEncoder(handle_unknown="ignore"), CAT),
        ("flag", Binarizer(threshold=0.5), FLAG),
        ("pass", "passthrough", PASS),
        ("gone", "drop", GONE)], remainder="drop", sparse_threshold=0.0)
    return ct.fit(X)


def sk_scaled_bound(y_sk):
    """The per-element bound of the module docstring for the 13 scaled columns (0 elsewhere)."""
    ct = sk_transformer()
    std, mm = ct.named_transformers_["num"].named_steps["std"], ct.named_transformers_["amt"].named_steps["mm"]
    so = np.zeros(OUT_WIDTH)
    so[0:10] = np.abs(std.mean_ / std.scale_)          # scale * offset, offset = mean_, scale = 1 / scale_
    so[10:13] = np.abs(mm.min_)                        # offset = -min_ / scale_, scale = scale_
    bound = ULP * (3 * np.abs(y_sk) + so)
    bound[:, 13:] = 0.0
    return bound


@functools.lru_cache(maxsize=None)
def sk_model(final="none"):
    """(fitted final estimator or None, ONNX model) of the pipeline: ``none`` ends at the assembled
    matrix, ``gbc`` a GradientBoostingClassifier, ``svc`` an RBF SVC exported raw ([dec, -dec]),
    ``svc_auto`` the same SVC exported as a classifier (label + probabilities)."""
    from igaming_platform_amd.onnx import convert
    ct = sk_transformer()
    if final == "none":
        return None, convert.column_pipeline(ct, N_FEAT)
    X, y, _ = sk_data()
    Z = ct.transform(X)
    if final == "gbc":
        from sklearn.ensemble import GradientBoostingClassifier
        est = GradientBoostingClassifier(n_estimators=30, max_depth=3, random_state=0).fit(Z, y)
        return est, convert.column_pipeline(ct, N_FEAT, final=est)
    from sklearn.svm import SVC
    est = SVC(kernel="rbf", C=1.0, gamma="scale").fit(Z, y)
    args = dict(output="raw") if final == "svc" else None
    return est, convert.column_pipeline(ct, N_FEAT, final=est, final_args=args)
