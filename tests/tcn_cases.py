"""Shared cases of the temporal-convolution (TCN) tests: a float64 numpy reference of the 1-D
convolution, the residual block and the read-outs, written from the formula

    out[o, t] = b[o] + sum_j sum_c W[o, c, j] * x[c, t - pad_left + j * dil]      (zero outside [0, T))

It reads a built model's initializers straight from the protobuf and calls neither the executor
nor the plan. ``torch_tcn`` is an independent evaluation on ``torch.nn.functional.conv1d`` (float64:
the check of the reference; float32: where the tolerance comes from)."""
from __future__ import annotations

import numpy as np

from igaming_platform_amd.onnx import builders

_NP = {1: np.float32, 7: np.int64, 6: np.int32}

# Absolute tolerance on a real-valued model's output (a probability) against the float64 reference:
# the largest error of the independent float32 evaluation (torch conv1d in float32) over REAL_MODELS,
# both layouts, on 256 rows each of real_input() and event_input() - 9.1e-8 measured on the CPU
# where this constant was recorded (f32_error(); another host's torch sums in another order: 1.17e-7 on the
# CPU of an MI355X machine) - times a margin of 4 for the device's different summation order.
# test_tcn.py::test_tolerance_derivation prints the host's figure and checks the constant against a float32
# evaluation in a fixed order, which gives the same figure on every host (fixed_order_f32_error(), 8.3e-8).
REAL_TOL = 3.6e-7
# The same tolerance holds between the device and the CPU executor (whose own error against the
# reference, executor_error(), is 7.8e-8: a deterministic figure, checked against REAL_TOL / 4).

DEFAULT_KW = dict()                                   # the builder's defaults: 2 blocks x 32 channels, k = 3, T = 100
WIDE_KW = dict(channels=(64, 64, 64, 64), dilations=(1, 2, 4, 8), seed=29)   # the typical abuse model
SHORT_KW = dict(seq=16)                               # the defaults over the last 16 events (the ring tests)
REAL_MODELS = {"default": DEFAULT_KW, "wide": WIDE_KW, "short": SHORT_KW}


def weights_of(m):
    """name -> array of a model's initializers (raw_data tensors, as the builders write them)."""
    return {t.name: np.frombuffer(t.raw_data, _NP[t.data_type]).reshape(tuple(t.dims)).copy() for t in m.graph.initializer}


def ref_conv(x, w, b, dil, pad_left, out_len=None):
    """x [N, C, T], w [M, C, k], b [M] or None -> [N, M, out_len (T)] in float64."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, C, T = x.shape
    M, _, k = w.shape
    L = T if out_len is None else out_len
    out = np.zeros((N, M, L)) + (0.0 if b is None else np.asarray(b, np.float64)[None, :, None])
    for j in range(k):
        for t in range(L):
            p = t - pad_left + j * dil
            if 0 <= p < T:
                out[:, :, t] += x[:, :, p] @ w[:, :, j].T
    return out


def ref_act(v, act):
    if act == "relu":
        return np.where(v > 0, v, 0.0)          # x > 0 ? x : 0, as the executor and the kernels: a NaN gives 0
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if act == "tanh":
        return np.tanh(v)
    return v


def ref_pool(x, op):
    """[N, C, T] -> [N, C]; max: a NaN in the column gives NaN (np.max propagates it)."""
    x = np.asarray(x, np.float64)
    if op == "last":
        return x[:, :, -1]
    if op == "mean":
        return x.sum(axis=2) / x.shape[2]
    if op == "sum":
        return x.sum(axis=2)
    return x.max(axis=2)


def to_nct(X, layout):
    """The model input ([T, N, I] layout 0, [N, T, I] layout 1) as [N, C, T]."""
    X = np.asarray(X)
    return X.transpose(0, 2, 1) if layout else X.transpose(1, 2, 0)


def _pad_left(k, d, causal):
    return d * (k - 1) if causal else (d * (k - 1)) // 2


def ref_tcn(m, X, channels=(32, 32), kernel=3, dilations=(1, 2), readout="last", layout=0, causal=True,
            residual=True, head=True, batch_norm=False, trace=None, **_):
    """The builder's network on the model input ``X`` in float64: [N, 1] probabilities or [N, C].
    ``trace``: a list that receives max |value| of every convolution's output and residual sum."""
    W = {k: v.astype(np.float64) for k, v in weights_of(m).items() if v.dtype == np.float32}
    x = to_nct(X, layout).astype(np.float64)

    def conv(tag, v, k, d, act=True):
        y = ref_conv(v, W[f"{tag}_W"], W[f"{tag}_B"], d, _pad_left(k, d, causal))
        if trace is not None:
            trace.append(float(np.abs(y).max()))
        if batch_norm and act:
            g, b, mu, var = (W[f"{tag}_bn_{n}"][None, :, None] for n in "gbmv")
            y = (y - mu) / np.sqrt(var + np.float64(np.float32(1e-5))) * g + b
        return ref_act(y, "relu") if act else y
    cin = x.shape[1]
    for bi, (cout, d) in enumerate(zip(channels, dilations)):
        h = conv(f"b{bi}c2", conv(f"b{bi}c1", x, kernel, d), kernel, d)
        if residual:
            skip = x if cin == cout else conv(f"b{bi}ds", x, 1, 1, act=False)
            if trace is not None:
                trace.append(float(np.abs(h + skip).max()))
            h = ref_act(h + skip, "relu")
        x, cin = h, cout
    p = ref_pool(x, readout)
    if not head:
        return p
    return ref_act(p @ W["Wh"] + W["Bh"], "sigmoid")


def torch_tcn(m, X, dtype, channels=(32, 32), kernel=3, dilations=(1, 2), readout="last", layout=0, causal=True,
              residual=True, head=True, **_):
    """The same network on torch.nn.functional.conv1d in ``dtype`` (an evaluation independent of
    ref_conv: explicit F.pad, then an unpadded dilated convolution)."""
    import torch
    import torch.nn.functional as F
    W = {k: torch.from_numpy(v).to(dtype) for k, v in weights_of(m).items() if v.dtype == np.float32}
    x = torch.from_numpy(np.ascontiguousarray(to_nct(X, layout))).to(dtype)

    def conv(tag, v, k, d, act=True):
        span = d * (k - 1)
        pl = _pad_left(k, d, causal)
        y = F.conv1d(F.pad(v, (pl, span - pl)), W[f"{tag}_W"], W[f"{tag}_B"], dilation=d)
        return torch.relu(y) if act else y
    cin = x.shape[1]
    for bi, (cout, d) in enumerate(zip(channels, dilations)):
        h = conv(f"b{bi}c2", conv(f"b{bi}c1", x, kernel, d), kernel, d)
        if residual:
            skip = x if cin == cout else conv(f"b{bi}ds", x, 1, 1, act=False)
            h = torch.relu(h + skip)
        x, cin = h, cout
    p = x[:, :, -1] if readout == "last" else x.mean(dim=2) if readout == "mean" else x.amax(dim=2)
    if head:
        p = torch.sigmoid(p @ W["Wh"] + W["Bh"])
    return p.numpy()


def real_input(layout, n=6, seq=100, in_dim=16, seed=3):
    """Event-like model input: values in [-1, 1], some histories short (zeros in front)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (seq, n, in_dim)).astype(np.float32)
    X[:seq // 2, 1] = 0.0
    X[:seq - 1, 2] = 0.0
    return np.ascontiguousarray(X.transpose(1, 0, 2)) if layout else X


def event_input(layout, n=256, seq=100, in_dim=16, seed=11):
    """Histories as the event rings hold them: bf16 values of mixed scale (amounts next to flags),
    right-aligned, lengths from 0 to more than ``seq``."""
    import torch
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((seq, n, in_dim)) * rng.choice([0.05, 1.0, 4.0], in_dim)
    for b, cnt in enumerate(rng.integers(0, seq + seq // 4, n)):
        X[:max(0, seq - int(cnt)), b] = 0.0
    X = torch.from_numpy(X.astype(np.float32)).to(torch.bfloat16).float().numpy()
    return np.ascontiguousarray(X.transpose(1, 0, 2)) if layout else X


def f32_error():
    """Largest |float32 torch evaluation - float64 reference| over REAL_MODELS, both layouts, on 256
    rows each of real_input() and event_input() (the two kinds of input the device tests feed)."""
    import torch
    worst = 0.0
    for kw in REAL_MODELS.values():
        seq = kw.get("seq", 100)
        for layout in (0, 1):
            m = builders.tcn(layout=layout, **kw)
            for X in (real_input(layout, n=256, seq=seq), event_input(layout, seq=seq)):
                worst = max(worst, float(np.abs(torch_tcn(m, X, torch.float32, layout=layout, **kw).astype(np.float64)
                                                - ref_tcn(m, X, layout=layout, **kw)).max()))
    return worst


def fixed_order_f32_tcn(m, X, channels=(32, 32), kernel=3, dilations=(1, 2), **_):
    """The builder's default-shaped network (causal, residual, last step, head; layout 0) in float32 numpy
    with elementwise operations only: every sum runs bias, then taps ascending, channels ascending, one
    rounding per multiply and per add - no BLAS, no fused multiply-add, so the result does not depend on the host."""
    f = np.float32
    W = {k: v for k, v in weights_of(m).items() if v.dtype == np.float32}
    x = np.ascontiguousarray(to_nct(X, 0), f)

    def conv(tag, v, k, d, act=True):
        w, b = W[f"{tag}_W"], W[f"{tag}_B"]
        N, Cn, T = v.shape
        vp = np.concatenate([np.zeros((N, Cn, d * (k - 1)), f), v], axis=2)
        out = np.broadcast_to(b[None, :, None], (N, w.shape[0], T)).astype(f).copy()
        for j in range(k):
            for c in range(Cn):
                out += w[None, :, c, j, None] * vp[:, c, None, j * d:j * d + T]
        return np.maximum(out, f(0)) if act else out
    cin = x.shape[1]
    for bi, (cout, d) in enumerate(zip(channels, dilations)):
        h = conv(f"b{bi}c2", conv(f"b{bi}c1", x, kernel, d), kernel, d)
        skip = x if cin == cout else conv(f"b{bi}ds", x, 1, 1, act=False)
        x, cin = np.maximum(h + skip, f(0)), cout
    p = x[:, :, -1]
    z = np.zeros(p.shape[0], f) + W["Bh"][0]
    for c in range(cin):
        z += p[:, c] * W["Wh"][c, 0]
    return (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(f)[:, None]


def fixed_order_f32_error(n=64):
    """Largest |fixed-order float32 evaluation - float64 reference| over REAL_MODELS on ``n`` rows each of
    real_input() and event_input()."""
    worst = 0.0
    for kw in REAL_MODELS.values():
        seq = kw.get("seq", 100)
        m = builders.tcn(**kw)
        for X in (real_input(0, n=n, seq=seq), event_input(0, n=n, seq=seq)):
            worst = max(worst, float(np.abs(fixed_order_f32_tcn(m, X, **kw).astype(np.float64) - ref_tcn(m, X, **kw)).max()))
    return worst


def executor_error():
    """The same figure for the CPU executor (float32 values between layers, sums in double)."""
    from igaming_platform_amd.native import native
    worst = 0.0
    for kw in REAL_MODELS.values():
        seq = kw.get("seq", 100)
        m = builders.tcn(**kw)
        ex = native().Executor(native().OnnxModel.from_bytes(m.SerializeToString()))
        for X in (real_input(0, n=256, seq=seq), event_input(0, seq=seq)):
            worst = max(worst, float(np.abs(ex.run({"input": X})["output"].astype(np.float64) - ref_tcn(m, X, **kw)).max()))
    return worst


def int_weights(lo=-2, hi=2):
    """A ``weights`` callable for builders.tcn: small integers, so sums of products of integer inputs
    stay exact in f32 as long as :func:`int_bound` says so."""
    return lambda shape, rng: rng.integers(lo, hi + 1, shape).astype(np.float32)


def int_bound(m, X, **kw):
    """An upper bound of every partial sum any evaluation order can meet in the integer model: the
    largest convolution output or residual sum of the network run on |x| with |W|, |b| (all values
    are then non-negative, so every partial sum is below its total and Relu changes nothing). Exact f32
    arithmetic needs it below 2^24."""
    W = weights_of(m)
    for t in m.graph.initializer:
        if t.data_type == 1:
            t.raw_data = np.abs(W[t.name]).astype(np.float32).tobytes()
    try:
        trace = []
        top = ref_tcn(m, np.abs(X), **dict(kw, head=False, readout="max", trace=trace))
        return max(trace + [float(top.max())])
    finally:
        for t in m.graph.initializer:
            if t.data_type == 1:
                t.raw_data = W[t.name].tobytes()


def int_conv_case(rng, rows, T, c_in, c_out, k, d):
    """One integer convolution layer: x [rows, T, c_in], W [c_out, c_in, k], b [c_out], all small
    integers (|sum| <= 3 * 2 * k * c_in + 4 < 2^24)."""
    x = rng.integers(-3, 4, (rows, T, c_in)).astype(np.float32)
    w = rng.integers(-2, 3, (c_out, c_in, k)).astype(np.float32)
    b = rng.integers(-4, 5, c_out).astype(np.float32)
    return x, w, b


def grid_sample():
    """(T, C_in, C_out, k, d, pad, rows) cases covering every listed value of every dimension of the
    issue's grid at least once; pad is 'zero' | 'causal' | 'half'. d = 0 stands for d (k - 1) >= T."""
    Ts, Cis, Cos, ks, ds = (1, 2, 15, 16, 17, 100), (1, 3, 16, 17), (1, 15, 16, 17, 33), (1, 2, 3), (1, 2, 4, 0)
    pads, rows = ("zero", "causal", "half"), (1, 63, 65)
    n = max(len(v) for v in (Ts, Cis, Cos, ks, ds, pads, rows))
    cases = []
    for i in range(2 * n):   # two passes with different strides, so the values meet in other combinations too
        s = 1 if i < n else 2
        pick = lambda v, o: v[(i * s + o) % len(v)]
        T, k = pick(Ts, 0), pick(ks, 1 + i // n)
        d = pick(ds, 2)
        if d == 0:
            k = max(k, 2)
            d = -(-T // (k - 1))
        cases.append((T, pick(Cis, 3), pick(Cos, 4), k, d, pick(pads, 5), pick(rows, 6)))
    return cases


def pad_of(kind, k, d):
    span = d * (k - 1)
    return 0 if kind == "zero" else span if kind == "causal" else span // 2
