"""Numpy oracle, cases and operands of the QDQ tests (tests/test_qdq.py on the CPU,
tests/test_qdq_gpu.py on the device).

The oracle is literal: the integer sum is exact (int64), the affine step v = acc * (s_x * s_w *
alpha) + bias is float64, then round half to even, then saturate. The device runs the affine
step in f32 (csrc/kernels/qgemm.hip); per element the oracle also gives the distance of v / s_y
from the nearest rounding tie and the bound 8 * 2^-24 * (|acc * mult| + |bias|) / s_y on the f32
epilogue's error in quanta (conversion, multiplier, product, sum and quotient roundings are five
half-ulp steps; 8 leaves room). An element closer to a tie than its bound is *ambiguous*: the
device may land one quantum away there. With power-of-two scales and biases on the multiplier's
grid every step is exact in f32 and the bytes must be equal, ties included."""
import numpy as np

Q_RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
Q_OFF = {"uint8": 128, "int8": 0}
UINT8_ZPS = (0, 3, 128, 255)
INT8_ZPS = (-128, 0, 5)
X_CONFIGS = [("uint8", z) for z in UINT8_ZPS] + [("int8", z) for z in INT8_ZPS]
EPS = 2.0 ** -24
GARBAGE = (0x7F, -0x80)      # bytes outside the live input block
SENTINEL_Q = 0x55            # int8 output buffers are filled with this


# ------------------------------------------------------------------------------ oracle
def quantize64(v, scale, zp, qtype):
    """QuantizeLinear in float64: saturate(round_half_even(v / scale) + zp), as int64."""
    lo, hi = Q_RANGE[qtype]
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(np.asarray(v, np.float64) / np.float64(scale)) + zp
    return np.clip(q, lo, hi).astype(np.int64)


def dequantize64(q, scale, zp):
    return (np.asarray(q, np.int64) - zp).astype(np.float64) * np.float64(scale)


def stored(q, qtype):
    """The device's byte of a quantised value: q - off as int8."""
    return (np.asarray(q, np.int64) - Q_OFF[qtype]).astype(np.int8)


def unstored(b, qtype):
    return np.asarray(b, np.int64) + Q_OFF[qtype]


def act64(name, z):
    z = np.asarray(z, np.float64)
    if name == "relu":
        return np.where(z > 0, z, 0.0)
    if name == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if name == "tanh":
        return np.tanh(z)
    assert name == "none", name
    return z


def qdense_oracle(xq, x_scale, x_zp, wq, w_scale, w_zp=0, bias=None, act="none", out=None, alpha=1.0):
    """One quantised dense layer. ``xq`` [M, K] and ``wq`` [N, K] are the quantised integers (not
    the stored bytes), ``w_scale`` one value or [N], ``out`` None or (s_y, z_y, type). Returns a
    dict: ``acc`` (int64), ``v`` (float64 after the activation), and with ``out`` also ``q``
    (int64), ``tie`` (distance of v / s_y from the nearest tie, in quanta), ``bound`` (the f32
    epilogue's error bound in quanta) and ``ambiguous`` (tie < bound)."""
    acc = ((np.asarray(xq, np.float64) - x_zp) @ (np.asarray(wq, np.float64) - w_zp).T)   # exact: |acc| < 2^53
    assert np.abs(acc).max(initial=0) < 2.0 ** 52
    mult = np.float64(np.float32(x_scale)) * np.asarray(w_scale, np.float32).astype(np.float64) * np.float64(alpha)
    b = np.zeros(acc.shape[1]) if bias is None else np.asarray(bias, np.float64)
    pre = acc * mult + b
    v = act64(act, pre)
    r = dict(acc=acc.astype(np.int64), v=v, err=8 * EPS * (np.abs(acc * mult) + np.abs(b)))
    if out is not None:
        s_y, z_y, t = out
        r["q"] = quantize64(v, s_y, z_y, t)
        u = v / np.float64(s_y)
        r["tie"] = np.abs(np.abs(u - np.floor(u)) - 0.5)
        r["bound"] = r["err"] / np.float64(s_y)
        r["ambiguous"] = r["tie"] < r["bound"]
    return r


# ------------------------------------------------------------------------------ layer cases
def _pow2(x):
    return np.float32(2.0 ** np.round(np.log2(x)))


def layer_case(M, N, K, x_type="uint8", x_zp=0, per_channel=False, w_uint8=False, out=None, act="none",
               pow2=False, seed=0):
    """Random operands of one layer: ``xq`` over the whole range of ``x_type``, int8 weights in
    [-127, 127] (``w_uint8``: stored uint8 with zero point 128), an int32-grid bias, and for
    ``out`` = "uint8" | "int8" an output scale under which about a tenth of the values saturate."""
    rng = np.random.default_rng(seed)
    lo, hi = Q_RANGE[x_type]
    xq = rng.integers(lo, hi + 1, (M, K))
    w = rng.integers(-127, 128, (N, K))
    s_x = np.float32(rng.uniform(0.004, 0.03))
    s_w = rng.uniform(0.5, 2.0, N if per_channel else 1).astype(np.float32) * np.float32(0.02 / np.sqrt(K))
    if pow2:
        s_x, s_w = _pow2(s_x), _pow2(s_w)
    mult = (np.float64(s_x) * s_w.astype(np.float64)).astype(np.float32)
    bq = rng.integers(-2000, 2001, N)
    bias = (bq * np.broadcast_to(mult, (N,)).astype(np.float64)).astype(np.float32)   # exact with pow2 scales
    c = dict(M=M, N=N, K=K, x_type=x_type, x_zp=int(x_zp), xq=xq, wq=w + (128 if w_uint8 else 0),
             w_zp=128 if w_uint8 else 0, x_scale=s_x, w_scale=np.broadcast_to(s_w, (N,)).copy(), bias=bias, act=act, out=None)
    if out is not None:
        v = qdense_oracle(xq, s_x, x_zp, c["wq"], c["w_scale"], c["w_zp"], bias, act)["v"]
        if act == "sigmoid":
            s_y, z_y = np.float32(2.0 ** -8 if pow2 else 1.0 / 255.0), Q_RANGE[out][0]
        else:
            s_y = np.float32(max(np.quantile(np.abs(v), 0.9), 1e-3) / (100.0 if act == "none" else 200.0))
            s_y = _pow2(s_y) if pow2 else s_y
            z_y = int(np.clip(Q_RANGE[out][0] + (128 if act == "none" else 3), *Q_RANGE[out]))
        c["out"] = (s_y, z_y, out)
    return c


def case_step(c):
    """The case as a models.plan.QDenseStep (what ``qdense_tables`` and the runner take)."""
    from igaming_platform_amd.models.plan import QDenseStep
    return QDenseStep(n=c["N"], k=c["K"], act=c["act"], wq_np=(c["wq"] - c["w_zp"]).astype(np.int32),
                      w_scale=np.asarray(c["w_scale"], np.float32), alpha=1.0, x_scale=c["x_scale"], x_zp=c["x_zp"],
                      x_type=c["x_type"], w_np=np.zeros((c["N"], c["K"]), np.float32), b_np=c["bias"], out_q=c["out"])


def case_oracle(c):
    return qdense_oracle(c["xq"], c["x_scale"], c["x_zp"], c["wq"], c["w_scale"], c["w_zp"], c["bias"], c["act"], c["out"])


def tables_eval(t, xq, x_type, n, k):
    """float64 value of the host tables on quantised inputs ``xq``: the device's arithmetic in
    exact integers and float64 (acc over the stored bytes, + corr, * mult, + bias)."""
    w8 = t["w8"].numpy().astype(np.int64)[:n, :k]
    acc = (np.asarray(xq, np.int64) - Q_OFF[x_type]) @ w8.T
    return ((acc + t["corr"].numpy().astype(np.int64)[None, :]).astype(np.float64)
            * t["mult"].numpy().astype(np.float64)[None, :] + t["bias"].numpy().astype(np.float64)[None, :])


# (M, N, K) of the tail test; the last row is the smallest batch launch_qgemm gives the 128 x 128 tile
TAIL_SHAPES = [(1, 1, 1), (37, 1, 30), (63, 15, 63), (65, 17, 65), (64, 64, 64), (130, 65, 129), (33, 130, 257),
               (4096, 128, 64)]
OUTS = (None, "uint8", "int8")
ACTS = ("none", "relu", "sigmoid")
GENERAL_SHAPE = (130, 65, 129)
GENERAL_SEEDS = (1, 2, 3, 4)
AMBIGUOUS_CAP = 1e-3        # at most this share of a general-scale case's elements


def tail_variants(shape_index):
    """The nine (output, activation) pairs of one shape, each with the next activation type / zero
    point of X_CONFIGS and alternating per-tensor / per-channel weights: every value of every
    option is met in every shape."""
    v = []
    for j, (out, act) in enumerate((o, a) for o in OUTS for a in ACTS):
        xt, xz = X_CONFIGS[(j + shape_index) % len(X_CONFIGS)]
        v.append(dict(x_type=xt, x_zp=xz, per_channel=bool((j + shape_index) & 1), w_uint8=j % 3 == 2, out=out, act=act))
    return v


# A sigmoid / tanh before the requantisation: the device's expf is good to a few ulp (relative
# 2.4e-7 on values below 1, so 256 * 2.4e-7 = 6e-5 quanta at s_y = 2^-8). Inside this margin of a
# rounding tie no f32 activation can promise the byte; such elements may be one quantum off.
ACT_TIE_MARGIN = 2e-4


def general_case(seed):
    return layer_case(*GENERAL_SHAPE, x_type="uint8", x_zp=(3, 128, 0, 255)[seed % 4], per_channel=True, out="uint8",
                      act="relu" if seed & 1 else "none", seed=500 + seed)


# ------------------------------------------------------------------------------ device operands
def garbage_input(M_alloc, ld, M, K, data):
    """int8 [M_alloc, ld] whose live block [:M, :K] is ``data`` and whose every other byte
    alternates 0x7F / 0x80: a kernel that lets a byte past K or past the live rows reach a sum
    moves it by +-127 x a weight."""
    import torch
    g = np.where((np.add.outer(np.arange(M_alloc), np.arange(ld)) & 1) == 0, GARBAGE[0], GARBAGE[1]).astype(np.int8)
    g[:M, :K] = data
    return torch.from_numpy(g)


def sentinel_q(M_alloc, ld):
    import torch
    return torch.full((M_alloc, ld), SENTINEL_Q, dtype=torch.int8)


def untouched_q(Y, M, N):
    import torch
    mask = torch.ones(Y.shape, dtype=torch.bool)
    mask[:M, :N] = False
    return bool(torch.all(Y.cpu()[mask] == SENTINEL_Q))


# ------------------------------------------------------------------------------ model cases
# ``qdq_mlp`` variants of the DeviceModel test: options, and the kinds the plan starts with
MODEL_VARIANTS = {"fused": (dict(), ["quant", "qdense"]), "unfused": (dict(hidden_act="LeakyRelu"), ["quant", "qdense", "row"]),
                  "trailing": (dict(out_qdq=True), ["quant", "qdense"])}
MODEL_WIDTHS = [(30, 64, 1), (33, 130, 17, 1)]
MODEL_BUCKETS = ((64, 37), (300, 300))     # (bucket, live rows)
MODEL_BAD_ROWS = 0.02                      # at most this share of a model case's rows may be ambiguous
# the inputs' seed: one for which every variant meets MODEL_BAD_ROWS (a condition on the inputs
# that tests/test_qdq.py checks on the CPU; with 147 hidden values per row and the bound of the
# module docstring, a 337-row case expects a handful of ambiguous rows)
MODEL_INPUT_SEED = 4000


def model_inputs(bucket, rows, width):
    return np.random.default_rng(MODEL_INPUT_SEED + bucket).uniform(-1.0, 2.0, (rows, width)).astype(np.float32)


def tree_qdq_model(seed=31):
    """TreeEnsembleRegressor (8 targets) -> Q -> DQ -> Gemm(DQ(W), DQ(b)) -> Sigmoid; the embedding is a
    second graph output, so the executor reports it."""
    from igaming_platform_amd.onnx import builders as B
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import ML_DOMAIN, model, node, tensor, tree_attrs, value_info
    rng = np.random.default_rng(seed)
    k = 8
    trees = [B.random_complete_tree(rng, 4, 30, k, leaf_scale=0.1) for _ in range(16)]
    wq = rng.integers(-127, 128, (k, 1)).astype(np.int8)
    s_x, s_w = np.float32(2.0 ** -7), np.float32(2.0 ** -6)
    inits = [tensor("xs", np.array(s_x, np.float32)), tensor("xz", np.array(128, np.uint8)), tensor("Wq", wq),
             tensor("ws", np.array(s_w, np.float32)), tensor("wz", np.array(0, np.int8)),
             tensor("Bq", np.array([40], np.int32)), tensor("bs", np.array(s_x * s_w, np.float32))]
    nodes = [node("TreeEnsembleRegressor", ["input"], ["emb"], domain=ML_DOMAIN, n_targets=k, aggregate_function="SUM",
                  post_transform="NONE", **tree_attrs(trees, "target")),
             node("QuantizeLinear", ["emb", "xs", "xz"], ["eq"]), node("DequantizeLinear", ["eq", "xs", "xz"], ["ed"]),
             node("DequantizeLinear", ["Wq", "ws", "wz"], ["Wd"]), node("DequantizeLinear", ["Bq", "bs"], ["Bd"]),
             node("Gemm", ["ed", "Wd", "Bd"], ["z"]), node("Sigmoid", ["z"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", 30])],
                 [value_info("emb", S.FLOAT, ["N", k]), value_info("output", S.FLOAT, ["N", 1])], inits,
                 name="tree_qdq", metadata={"family": "stacked"})


# ------------------------------------------------------------------------------ model oracle
def model_oracle(plan, X, trace=None):
    """float64 walk of a compiled chain plan whose steps are quant / qdense / dequant / row (leaky
    relu) - the plans of the ``qdq_mlp`` variants. Returns (output [M, out], ambiguous rows);
    ``trace`` (a list) receives the quantised integers of every quantised step output in order."""
    h = np.asarray(X, np.float64)
    err = np.zeros_like(h)    # bound on the device's f32 error of h (the model input is exact)
    bad = np.zeros(h.shape[0], bool)
    q = None
    for s in plan.steps:
        if s.kind == "quant":
            u = h / np.float64(s.scale)
            # the device divides its f32 value in f32: h's own error plus one rounding of the quotient
            bad |= (np.abs(np.abs(u - np.floor(u)) - 0.5) < err / np.float64(s.scale) + 2 * EPS * np.abs(u)).any(axis=1)
            q = quantize64(h, s.scale, s.zp, s.qtype)
            if trace is not None:
                trace.append(q)
        elif s.kind == "qdense":
            r = qdense_oracle(q, s.x_scale, s.x_zp, s.wq_np, s.w_scale, 0, s.b_np, s.act, s.out_q, s.alpha)
            if s.out_q is not None:
                amb = r["ambiguous"]
                if s.act in ("sigmoid", "tanh"):
                    amb = amb | (r["tie"] < ACT_TIE_MARGIN)
                bad |= amb.any(axis=1)
                q = r["q"]
                if trace is not None:
                    trace.append(q)
            else:
                h, err = r["v"], r["err"]
        elif s.kind == "dequant":
            h = dequantize64(q, s.scale, s.zp)
            err = np.zeros_like(h)
        else:
            assert s.kind == "row" and s.op == "act" and s.act == "leaky_relu", s.kind
            h = np.where(h > 0, h, np.float64(np.float32(s.p0)) * h)
            err = err + EPS * np.abs(h)
    return h, bad
