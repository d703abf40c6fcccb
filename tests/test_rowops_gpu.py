"""csrc/kernels/rowops.hip on the device: layernorm, softmax and every elementwise activation
against the float64 references of tests/row_cases.py at every width around the kernels' chunk,
wave and instantiation boundaries, with the scalar and the vector load paths, live rows given as M
and through m_ptr, and all f32 / bf16 operand combinations; then the framework-style models that
lower to row steps through DeviceModel, the engine (direct launch and graph replay) and the LTV
service.

Inputs sit in buffers whose stride padding is NaN and outputs in buffers pre-filled with -7 that
must stay bit-identical outside the live block: a kernel that reads past N or writes past N / the
live rows fails the comparison, no fault needed.

Tolerances: f32 outputs 1e-5 absolute and relative against float64 (the same two-pass f32
arithmetic on the host stays within 3.5e-7 of float64 on these inputs); bf16 outputs within one
bf16 ulp of the float64 result rounded to bf16; device models 1e-5 (fp32) and 3e-2 (bf16) against
the C++ executor, as tests/test_onnx_ml_gpu.py."""
from functools import lru_cache

import numpy as np
import pytest

from tests import row_cases as R

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-5)
OPS = ["layernorm", "softmax"] + list(R.ACTS)


def _t():
    import torch
    return torch


def _K():
    from igaming_platform_amd.ops import kernels as K
    return K


def _i32(v):
    torch = _t()
    return torch.tensor([v], dtype=torch.int32, device="cuda")


@lru_cache(maxsize=None)
def _case(op, N, xbf=False):
    """(X, gamma, beta, float64 reference) of one op at one width; computed once, never changed."""
    X = R.inputs(N)
    if xbf:
        X = R.bf16r(X).astype(np.float32)   # the values a bf16 operand holds
    gam, bet = R.affine(N)
    if op == "layernorm":
        ref = R.ref_layernorm(X, gam, bet)
    elif op == "softmax":
        ref = R.ref_softmax(X)
    else:
        ref = R.ref_act(op, X, *R.ACTS[op], slope=0.2 * gam if op == "prelu" else None)
    for a in (X, gam, bet, ref):
        a.setflags(write=False)
    return X, gam, bet, ref


def _launch(op, Xd, Y, M, N, gam, bet, m_ptr=None):
    K = _K()
    if op == "layernorm":
        K.row_op("layernorm", Xd, Y, M, N, eps=R.EPS, gamma=gam, beta=bet, m_ptr=m_ptr)
    elif op == "softmax":
        K.row_op("softmax", Xd, Y, M, N, m_ptr=m_ptr)
    else:
        p0, p1 = R.ACTS[op]
        K.row_op("act", Xd, Y, M, N, act=op, p0=p0, p1=p1, gamma=0.2 * gam if op == "prelu" else None, m_ptr=m_ptr)


def _operand(X, ld, dtype):
    """[ROWS_ALLOC, ld] device tensor: X in [:rows, :N], NaN in the stride padding and below."""
    torch = _t()
    t = torch.full((R.ROWS_ALLOC, ld), float("nan"), dtype=dtype)
    t[:X.shape[0], :X.shape[1]] = torch.tensor(X).to(dtype)
    return t.cuda()


def _untouched(Y, live, N):
    torch = _t()
    mask = torch.ones(Y.shape, dtype=torch.bool, device=Y.device)
    mask[:live, :N] = False
    bits = {2: torch.int16, 4: torch.int32}[Y.element_size()]
    want = torch.full((), R.SENTINEL, dtype=Y.dtype, device=Y.device).view(bits)
    return bool(torch.all(Y.view(bits)[mask] == want))


# ------------------------------------------------------------------------------ kernel vs float64
@pytest.mark.parametrize("N", R.WIDTHS)
@pytest.mark.parametrize("op", OPS)
def test_row_op_matches_float64(op, N):
    """f32 in / out: every stride (ld = N, N + 3: scalar loads; the next multiple of 8: 16-byte
    loads with a scalar tail chunk), 1 / 5 / 67 live rows of 128 given as M and through m_ptr."""
    torch = _t()
    X, gam, bet, ref = _case(op, N)
    gd, bd = torch.tensor(gam).cuda(), torch.tensor(bet).cuda()
    for ld in R.strides(N):
        Xd = _operand(X, ld, torch.float32)
        for live in R.LIVE:
            for by_ptr in (False, True):
                Y = torch.full((R.ROWS_ALLOC, ld), R.SENTINEL, dtype=torch.float32, device="cuda")
                if by_ptr:
                    _launch(op, Xd, Y, R.ROWS_ALLOC, N, gd, bd, m_ptr=_i32(live))
                else:
                    _launch(op, Xd, Y, live, N, gd, bd)
                where = f"{op} N={N} ld={ld} live={live} m_ptr={by_ptr}"
                assert _untouched(Y, live, N), where + ": wrote outside the live block"
                np.testing.assert_allclose(Y[:live, :N].cpu().numpy(), ref[:live], err_msg=where, **TOL)


@pytest.mark.parametrize("ybf", [False, True], ids=["yf32", "ybf16"])
@pytest.mark.parametrize("xbf", [False, True], ids=["xf32", "xbf16"])
@pytest.mark.parametrize("N", R.MIXED_WIDTHS)
@pytest.mark.parametrize("op", OPS)
def test_row_op_mixed_dtypes(op, N, xbf, ybf):
    """All four f32 / bf16 input / output combinations on both load paths. A bf16 output is the f32
    result rounded once: within one bf16 ulp of the float64 result rounded to bf16."""
    torch = _t()
    X, gam, bet, ref = _case(op, N, xbf)
    gd, bd = torch.tensor(gam).cuda(), torch.tensor(bet).cuda()
    live = 67
    for ld in R.strides(N):
        Xd = _operand(X, ld, torch.bfloat16 if xbf else torch.float32)
        Y = torch.full((R.ROWS_ALLOC, ld), R.SENTINEL, dtype=torch.bfloat16 if ybf else torch.float32, device="cuda")
        _launch(op, Xd, Y, R.ROWS_ALLOC, N, gd, bd, m_ptr=_i32(live))
        assert _untouched(Y, live, N), f"ld={ld}: wrote outside the live block"
        got = Y[:live, :N].float().cpu().numpy().astype(np.float64)
        if ybf:
            want = R.bf16r(ref)
            assert np.all(np.abs(got - want) <= R.bf16_ulp(want)), f"ld={ld}: {np.abs(got - want).max()}"
        else:
            np.testing.assert_allclose(got, ref, err_msg=f"ld={ld}", **TOL)


# ------------------------------------------------------------------------------ special rows
def _run_f32(op, X, N=None, **kw):
    torch, K = _t(), _K()
    X = np.ascontiguousarray(X, np.float32)
    N = N or X.shape[1]
    Xd = torch.from_numpy(X).cuda()
    Y = torch.full(X.shape, R.SENTINEL, dtype=torch.float32, device="cuda")
    K.row_op(op, Xd, Y, X.shape[0], N, **kw)
    return Y.cpu().numpy()


@pytest.mark.parametrize("N", [2, 64, 300, 1500])
def test_softmax_large_and_equal_rows(N):
    rng = np.random.default_rng(N)
    X = np.stack([1e4 * rng.standard_normal(N), np.full(N, 1e4), np.full(N, -3.25), -1e4 * np.ones(N)]).astype(np.float32)
    Y = _run_f32("softmax", X)
    assert np.all(np.isfinite(Y))
    np.testing.assert_allclose(Y.astype(np.float64).sum(axis=1), 1.0, rtol=1e-6)
    np.testing.assert_allclose(Y[0], R.ref_softmax(X[:1])[0], **TOL)
    np.testing.assert_allclose(Y[1:], np.float32(1.0) / np.float32(N), rtol=2e-7, atol=0)   # all-equal rows: 1 / N


def test_layernorm_constant_row_returns_beta():
    torch = _t()
    N = 64
    gam, bet = R.affine(N)
    X = R.inputs(N, 8).copy()
    X[3] = 12.625
    Y = _run_f32("layernorm", X, gamma=torch.from_numpy(gam).cuda(), beta=torch.from_numpy(bet).cuda(), eps=R.EPS)
    np.testing.assert_array_equal(Y[3], bet)   # zero deviations: exactly beta
    np.testing.assert_allclose(Y[[0, 1, 2, 4, 5, 6, 7]], R.ref_layernorm(X, gam, bet)[[0, 1, 2, 4, 5, 6, 7]], **TOL)
    # beta is optional
    Y = _run_f32("layernorm", X, gamma=torch.from_numpy(gam).cuda(), eps=R.EPS)
    np.testing.assert_allclose(np.delete(Y, 3, 0), np.delete(R.ref_layernorm(X, gam), 3, 0), **TOL)
    assert not Y[3].any()


@pytest.mark.parametrize("op", ["layernorm", "softmax"])
@pytest.mark.parametrize("N", [65, 600, 1100])
def test_nan_row_changes_no_other_row(op, N):
    torch = _t()
    gam = torch.from_numpy(R.affine(N)[0]).cuda()
    kw = dict(gamma=gam, eps=R.EPS) if op == "layernorm" else {}
    X = R.inputs(N, 9).copy()
    clean = _run_f32(op, X, **kw)
    X[4, N // 2] = np.nan   # row 4 shares its block with rows 5 - 7
    Y = _run_f32(op, X, **kw)
    assert np.all(np.isnan(Y[4]))
    np.testing.assert_array_equal(np.delete(Y, 4, 0), np.delete(clean, 4, 0))


def test_activations_are_overflow_safe():
    X = np.array([[-100.0, 100.0, -10.0, 10.0, 0.0]], np.float32)
    sp = _run_f32("act", X, act="softplus")[0]
    np.testing.assert_allclose(sp, R.ref_act("softplus", X)[0], **TOL)
    assert sp[1] == 100.0 and 0.0 <= sp[0] < 1e-40 and np.all(np.isfinite(sp))
    el = _run_f32("act", X, act="elu", p0=1.0)[0]
    assert el[0] == -1.0 and el[1] == 100.0
    se = _run_f32("act", X, act="selu", p0=R.ACTS["selu"][0], p1=R.ACTS["selu"][1])[0]
    np.testing.assert_allclose(se, R.ref_act("selu", X, *R.ACTS["selu"])[0], **TOL)
    for act in ("gelu", "gelu_tanh"):
        ge = _run_f32("act", X, act=act)[0]
        assert np.all(np.isfinite(ge)) and ge[3] == 10.0 and abs(ge[2]) < 1e-20 and ge[1] == 100.0 and ge[0] == 0.0
    sg = _run_f32("act", X, act="sigmoid")[0]
    assert sg[0] >= 0.0 and sg[1] == 1.0 and np.all(np.isfinite(sg))


def test_row_op_validates_operands():
    torch, K = _t(), _K()
    X = torch.zeros((8, 16), device="cuda")
    Y = torch.zeros((8, 16), device="cuda")
    g = torch.ones(16, device="cuda")
    for kw, msg in ((dict(op="layernorm"), "needs gamma"), (dict(op="norm"), "op must be"),
                    (dict(op="act", act="swish"), "act must be"), (dict(op="softmax", gamma=g), "gamma is read"),
                    (dict(op="softmax", N=17), "smaller than"), (dict(op="softmax", M=9), "smaller than"),
                    (dict(op="layernorm", gamma=g[:8]), "elements"), (dict(op="layernorm", gamma=g.double()), "dtype")):
        kw = dict(dict(M=8, N=16), **kw)
        with pytest.raises(ValueError, match=msg):
            K.row_op(kw.pop("op"), X, Y, kw.pop("M"), kw.pop("N"), **kw)
    with pytest.raises(ValueError, match="2-D float32 or bfloat16"):
        K.row_op("softmax", X.half(), Y, 8, 16)
    K.row_op("softmax", X, Y, 0, 16)   # no live rows: nothing launched
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ plans vs executor
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,kw,kinds", R.MODEL_CASES, ids=[R.model_id(c) for c in R.MODEL_CASES])
def test_device_plan_matches_executor(kind, kw, kinds, precision):
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    N = native()
    om = N.OnnxModel.from_bytes(builders.build(kind, **kw).SerializeToString())
    plan = to_device(compile_onnx(om), "cuda", precision=precision)
    assert [s.kind for s in plan.steps] == kinds
    dm = DeviceModel(plan, "cuda", [64, 512])
    if precision == "bf16":   # a row step between two MFMA layers passes bf16 activations on
        for i, s in enumerate(plan.steps[:-1]):
            if s.kind == "row" and all(plan.steps[j].kind in ("dense", "head", "join", "row") for j in dm.consumers[i]):
                assert dm.step_out[i].dtype == torch.bfloat16
    rng = np.random.default_rng(11)
    for rows in (1, 37, 512):
        X = rng.standard_normal((rows, kw["n_features"])).astype(np.float32)
        ref = np.asarray(N.Executor(om).run({"input": X})["output"]).reshape(rows, -1)[:, plan.executor_col]
        Xd = torch.zeros((512, kw["n_features"]), dtype=torch.float32, device="cuda")
        Xd[:rows] = torch.from_numpy(X).cuda()
        bucket = 64 if rows <= 64 else 512
        out = dm.run(Xd, bucket)
        torch.cuda.synchronize()
        got = out[:rows, plan.ml_col].float().cpu().numpy()
        tol = 1e-5 if precision == "fp32" else 3e-2
        np.testing.assert_allclose(got, ref, atol=tol, rtol=tol)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("n_out", [2, 5, 300])
def test_device_softmax_row_step_matches_executor(n_out, precision):
    """Softmax that cannot narrow (logits behind a Tanh row step / wider than two) runs as a row
    step; two columns report the positive class in column 1 on both sides."""
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    N = native()
    rng = np.random.default_rng(n_out)
    w1 = (rng.standard_normal((30, 48)) / np.sqrt(30)).astype(np.float32)
    w2 = (rng.standard_normal((48, n_out)) / np.sqrt(48)).astype(np.float32)
    m = model([node("MatMul", ["input", "W1"], ["h"]), node("Relu", ["h"], ["a"]), node("MatMul", ["a", "W2"], ["z"]),
               node("Tanh", ["z"], ["t"]), node("Tanh", ["t"], ["t2"]), node("Softmax", ["t2"], ["output"], axis=1)],
              [value_info("input", S.FLOAT, ["N", 30])], [value_info("output", S.FLOAT, ["N", n_out])],
              [tensor("W1", w1), tensor("W2", w2)])
    om = N.OnnxModel.from_bytes(m.SerializeToString())
    plan = to_device(compile_onnx(om), "cuda", precision=precision)
    assert [s.kind for s in plan.steps] == ["dense", "dense", "row", "row"] and plan.steps[-1].op == "softmax"
    assert plan.ml_col == plan.executor_col == (1 if n_out == 2 else 0)
    dm = DeviceModel(plan, "cuda", [64])
    X = rng.standard_normal((37, 30)).astype(np.float32)
    ref = np.asarray(N.Executor(om).run({"input": X})["output"])
    Xd = torch.zeros((64, 30), dtype=torch.float32, device="cuda")
    Xd[:37] = torch.from_numpy(X).cuda()
    got = dm.run(Xd, 64)[:37].float().cpu().numpy()
    tol = 1e-5 if precision == "fp32" else 3e-2
    np.testing.assert_allclose(got, ref, atol=tol, rtol=tol)


# ------------------------------------------------------------------------------ engine and LTV
@pytest.mark.parametrize("direct", ["1", "0"], ids=["direct", "graph"])
@pytest.mark.parametrize("kind,kw", [("torch_mlp", dict(act="Relu", out=2)), ("torch_mlp", dict(act="LeakyRelu", out=2)),
                                     ("tabular_resnet", dict(norm="layer")), ("tabular_resnet", dict(norm="batch"))],
                         ids=["torch_mlp-relu", "torch_mlp-leaky", "resnet-layer", "resnet-batch"])
def test_engine_gpu_matches_cpu(kind, kw, direct, monkeypatch):
    """The scorer's recorded direct launches and its graph replay both carry the row steps."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.onnx import builders
    from tests.test_engine_cpu import NOW, _txs
    monkeypatch.setenv("IGP_DIRECT_LAUNCH", direct)
    m = builders.build(kind, n_features=30, **kw).SerializeToString()
    cfg = Config()
    cfg.gpu.buckets = [64, 256]
    cfg.gpu.max_batch = 256
    g = RiskEngine(cfg, backend="gpu", capacity=512, fraud_model=m)
    c = RiskEngine(cfg, backend="cpu", capacity=512, fraud_model=m)
    txs = _txs(200, np.random.default_rng(12))
    a, b = g.score(txs, now=NOW), c.score(txs, now=NOW)
    np.testing.assert_allclose([x["ml_score"] for x in a], [x["ml_score"] for x in b], atol=1e-5)
    assert np.ptp([x["ml_score"] for x in a]) > 1e-3
    g.close()
    c.close()


def test_narrowed_two_logit_mlp_fuses_the_ensemble():
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    N = native()
    for act, fuses in (("Relu", True), ("LeakyRelu", False)):
        om = N.OnnxModel.from_bytes(builders.torch_mlp(n_features=30, act=act, out=2).SerializeToString())
        dm = DeviceModel(to_device(compile_onnx(om), "cuda"), "cuda", [64])
        assert dm.fuses_ensemble() == fuses, dm.plan.describe()


def _ltv_layernorm_model(n_features=64, width=64, seed=21):
    """Gemm -> LayerNormalization -> Relu -> Gemm -> output [N, 1]: an LTV regressor with a norm."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    rng = np.random.default_rng(seed)
    gam, bet = R.affine(width)
    inits = [tensor("W0", (rng.standard_normal((n_features, width)) * np.sqrt(2.0 / n_features)).astype(np.float32)),
             tensor("B0", (rng.standard_normal(width) * 0.01).astype(np.float32)), tensor("g", gam), tensor("b", bet),
             tensor("W1", (rng.standard_normal((width, 1)) * 40.0 / np.sqrt(width)).astype(np.float32)),
             tensor("B1", np.array([150.0], np.float32))]
    nodes = [node("Gemm", ["input", "W0", "B0"], ["h"]), node("LayerNormalization", ["h", "g", "b"], ["n"], axis=-1),
             node("Relu", ["n"], ["a"]), node("Gemm", ["a", "W1", "B1"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])], [value_info("output", S.FLOAT, ["N", 1])],
                 inits, name="ltv_layernorm", metadata={"family": "mlp"})


def test_gpu_ltv_with_layernorm_matches_cpu():
    """An LTV model with a LayerNormalization is no dense chain: the service runs it step by step
    through DeviceModel (dense -> layernorm -> relu -> dense) and answers as the CPU backend does,
    at the tolerance of tests/test_engine_gpu.py::test_gpu_ltv_matches_cpu."""
    from igaming_platform_amd.golden import ltv as GL
    from tests.test_engine_gpu import _engines
    m = _ltv_layernorm_model().SerializeToString()
    g, c = _engines(ltv_model=m)
    ltv = g.ltv.gpu[0]
    assert ltv.chain is None and [s.kind for s in ltv.plan.steps] == ["dense", "row", "row", "dense"]
    rng = np.random.default_rng(4)
    players = [GL.PlayerFeatures(days_since_registration=int(rng.integers(1, 900)),
                                 days_since_last_bet=int(rng.integers(0, 60)),
                                 days_since_last_deposit=int(rng.integers(0, 90)),
                                 sessions_per_week=float(rng.uniform(0, 8)), net_revenue=float(rng.uniform(-500, 30000)),
                                 deposit_frequency=float(rng.uniform(0, 6)), bet_count=int(rng.integers(0, 400)),
                                 support_tickets=int(rng.integers(0, 6))) for _ in range(100)]
    ids = [f"p{i}" for i in range(100)]
    for e in (g, c):
        e.set_players(ids, players)
    rg, rc = g.predict_ltv_batch(ids), c.predict_ltv_batch(ids)
    for x, y in zip(rg, rc):
        assert x.churn_risk == pytest.approx(y.churn_risk) and x.survival_days == y.survival_days
        assert x.predicted_ltv == pytest.approx(y.predicted_ltv, rel=3e-2, abs=1.0)
        assert x.confidence == pytest.approx(y.confidence)
    assert np.ptp([x.predicted_ltv for x in rg]) > 10.0
    g.close()
    c.close()
