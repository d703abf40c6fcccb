"""Cases, operands and float64 references for the row-op tests (tests/test_rowops_cpu.py on the
CPU executor and the plan lowering, tests/test_rowops_gpu.py on the device): layernorm, softmax
and the elementwise activations of csrc/kernels/rowops.hip, and the framework-style models that
lower to them.

Inputs are 3 x N(0, 1) plus a per-row offset in [-2, 2] (fixed seeds): rows with a mean of their
own, values out to about +-15. The references are plain float64 numpy / scipy."""
import numpy as np
from scipy.special import erfc

from tests.dense_cases import SENTINEL, bf16r  # noqa: F401  (shared conventions)

# every vector / scalar path and instantiation boundary of the kernels: below one chunk, one chunk,
# around one wave's 64 lanes, around 256 / 512 / 1024 (1 / 2 / 4 float4 per lane), the looped kernel
WIDTHS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 1500)
ROWS_ALLOC = 128
LIVE = (1, 5, 67)            # one wave; a partial block of 4; 16 full blocks + 3 waves
MIXED_WIDTHS = (65, 256)     # all four f32 / bf16 input / output combinations
EPS = 1e-5


def strides(N):
    """N itself, N + 3 (rows off every 8- / 16-byte boundary: the scalar path) and the next
    multiple of 8 above N (aligned rows wider than N: the vector path)."""
    return (N, N + 3, (N // 8 + 1) * 8)


# act -> (p0, p1): the ONNX defaults, except where the default makes the op trivial
ACTS = {"relu": (0.0, 0.0), "sigmoid": (0.0, 0.0), "tanh": (0.0, 0.0), "leaky_relu": (0.01, 0.0),
        "elu": (1.0, 0.0), "selu": (1.67326319217681884765625, 1.05070102214813232421875),
        "softplus": (0.0, 0.0), "hard_sigmoid": (0.2, 0.5), "gelu": (0.0, 0.0), "gelu_tanh": (0.0, 0.0),
        "clip": (-1.5, 2.25), "prelu": (0.25, 0.0)}


def inputs(N, rows=max(LIVE), seed=0):
    rng = np.random.default_rng(7000 + 13 * N + seed)
    return (3.0 * rng.standard_normal((rows, N)) + rng.uniform(-2, 2, (rows, 1))).astype(np.float32)


def affine(N):
    """(gamma, beta) of a layernorm / per-column PRelu slopes: gamma in [0.5, 1.5]."""
    rng = np.random.default_rng(7100 + N)
    return rng.uniform(0.5, 1.5, N).astype(np.float32), (0.5 * rng.standard_normal(N)).astype(np.float32)


# ------------------------------------------------------------------------------ references
def ref_layernorm(X, gamma, beta=None, eps=EPS):
    X = np.asarray(X, np.float64)
    mu = X.mean(axis=1, keepdims=True)
    var = ((X - mu) ** 2).mean(axis=1, keepdims=True)
    y = (X - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64)
    return y if beta is None else y + np.asarray(beta, np.float64)


def ref_softmax(X):
    X = np.asarray(X, np.float64)
    e = np.exp(X - X.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def ref_act(act, X, p0=0.0, p1=0.0, slope=None):
    x = np.asarray(X, np.float64)
    p0, p1 = float(np.float32(p0)), float(np.float32(p1))   # the parameters travel as f32
    with np.errstate(over="ignore"):
        if act == "relu":
            return np.where(x > 0, x, 0.0)
        if act == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if act == "tanh":
            return np.tanh(x)
        if act == "leaky_relu":
            return np.where(x > 0, x, p0 * x)
        if act == "elu":
            return np.where(x > 0, x, p0 * np.expm1(np.minimum(x, 0)))
        if act == "selu":
            return p1 * np.where(x > 0, x, p0 * np.expm1(np.minimum(x, 0)))
        if act == "softplus":
            return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
        if act == "hard_sigmoid":
            return np.clip(p0 * x + p1, 0.0, 1.0)
        # x Phi(x) and 0.5 x (1 + tanh(u)) = x sigmoid(2u), in the forms that keep the negative tail
        # (1 + erf and 1 + tanh cancel there, in float64 too: below about -8.3 they return 0)
        if act == "gelu":
            return 0.5 * x * erfc(-x / np.sqrt(2.0))
        if act == "gelu_tanh":
            return x / (1.0 + np.exp(-2.0 * np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
        if act == "clip":
            return np.clip(x, p0, p1)
        if act == "prelu":
            return np.where(x >= 0, x, (p0 if slope is None else np.asarray(slope, np.float64)) * x)
    raise AssertionError(act)


def bf16_ulp(a):
    """One bfloat16 unit in the last place at each value of ``a`` (8 significant bits)."""
    a = np.maximum(np.abs(np.asarray(a, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


# ------------------------------------------------------------------------------ models
# (builder, kwargs, step kinds of the lowered plan)
MODEL_CASES = [
    ("torch_mlp", dict(n_features=30, hidden=64, layers=1, act="Relu", out=2), ["head"]),
    ("torch_mlp", dict(n_features=30, hidden=64, layers=2, act="Relu", out=1), ["dense", "head"]),
    ("torch_mlp", dict(n_features=30, hidden=64, layers=2, act="LeakyRelu", out=2),
     ["dense", "row", "dense", "row", "dense"]),
    ("torch_mlp", dict(n_features=30, hidden=100, layers=1, act="LeakyRelu", out=1), ["dense", "row", "dense"]),
    ("tabular_resnet", dict(n_features=30, width=64, blocks=2, norm="layer"),
     ["dense", "row", "dense", "dense", "join", "row", "row", "dense", "dense", "join", "row", "row", "row", "dense"]),
    ("tabular_resnet", dict(n_features=30, width=64, blocks=2, norm="batch"),
     ["dense", "dense", "dense", "join", "row", "dense", "dense", "join", "row", "head"]),
]


def model_id(c):
    return "-".join([c[0]] + [str(v) for k, v in c[1].items() if k != "n_features"])
