"""Framework-exported MLPs on the host: the C++ executor's normalisations and activations
(BatchNormalization, LayerNormalization, Dropout, Elu, Selu, Softplus, HardSigmoid, Gelu, PRelu)
against float64 torch / numpy, and the lowering of those models (models/plan.py RowStep,
BatchNormalization folded like a Scaler, a two-logit Softmax narrowed to the fused head): the
lowered plan is evaluated with numpy and compared with the executor - the same math
csrc/kernels/rowops.hip runs (tests/test_rowops_gpu.py runs it on the device)."""
import numpy as np
import pytest

from igaming_platform_amd.models.plan import PlanError, compile_onnx, executor_output, step_inputs
from igaming_platform_amd.native import native
from igaming_platform_amd.onnx import builders
from igaming_platform_amd.onnx import schema as S
from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
from tests import row_cases as R

N = native()
TOL_EXEC = 2e-6   # executor against float64: the bound of tests/test_lstm_cpu.py


def _load(m):
    return N.OnnxModel.from_bytes(m.SerializeToString())


def _graph(nodes, width, inits=(), out_width=None, outputs=("output",)):
    return model(nodes, [value_info("input", S.FLOAT, ["N", width])],
                 [value_info(o, S.FLOAT, ["N", out_width or width]) for o in outputs], list(inits))


def _run(m, X):
    return N.Executor(_load(m)).run({"input": np.ascontiguousarray(X, np.float32)})


def _x(width=37, rows=50, seed=0):
    return R.inputs(width, rows, seed)


def _t64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.float64))


# ------------------------------------------------------------------------------ executor ops
@pytest.mark.parametrize("eps", [None, 1e-3])
def test_executor_batch_norm_matches_torch(eps):
    import torch.nn.functional as F
    rng = np.random.default_rng(1)
    C = 37
    s, b = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    mu, var = rng.standard_normal(C).astype(np.float32), rng.uniform(0.1, 3.0, C).astype(np.float32)
    attrs = {} if eps is None else dict(epsilon=eps)
    g = _graph([node("BatchNormalization", ["input", "s", "b", "m", "v"], ["output"], **attrs)], C,
               [tensor("s", s), tensor("b", b), tensor("m", mu), tensor("v", var)])
    X = _x(C)
    e = float(np.float32(1e-5 if eps is None else eps))
    want = F.batch_norm(_t64(X), _t64(mu), _t64(var), _t64(s), _t64(b), training=False, eps=e).numpy()
    assert float(np.abs(_run(g, X)["output"] - want).max()) <= TOL_EXEC


@pytest.mark.parametrize("bias", [True, False])
def test_executor_layer_norm_matches_torch(bias):
    import torch.nn.functional as F
    C = 37
    gam, bet = R.affine(C)
    ins = ["input", "g"] + (["b"] if bias else [])
    g = _graph([node("LayerNormalization", ins, ["output"], axis=-1)], C, [tensor("g", gam), tensor("b", bet)])
    X = _x(C)
    want = F.layer_norm(_t64(X), (C,), _t64(gam), _t64(bet) if bias else None, eps=float(np.float32(1e-5))).numpy()
    assert float(np.abs(_run(g, X)["output"] - want).max()) <= TOL_EXEC


def _torch_act(name):
    import torch.nn.functional as F
    return {"Elu": lambda x: F.elu(x, alpha=1.0), "Selu": F.selu, "Softplus": F.softplus,
            "Gelu": F.gelu, "GeluTanh": lambda x: F.gelu(x, approximate="tanh")}[name]


@pytest.mark.parametrize("name", ["Elu", "Selu", "Softplus", "Gelu", "GeluTanh"])
def test_executor_activations_match_torch(name):
    op, attrs = ("Gelu", dict(approximate="tanh")) if name == "GeluTanh" else (name, {})
    X = _x()
    got = _run(_graph([node(op, ["input"], ["output"], **attrs)], X.shape[1]), X)["output"]
    want = _torch_act(name)(_t64(X)).numpy()
    assert float(np.abs(got - want).max()) <= TOL_EXEC


def test_executor_elu_alpha_and_hard_sigmoid_defaults():
    X = _x()
    got = _run(_graph([node("Elu", ["input"], ["output"], alpha=0.5)], X.shape[1]), X)["output"]
    assert float(np.abs(got - R.ref_act("elu", X, 0.5)).max()) <= TOL_EXEC
    got = _run(_graph([node("HardSigmoid", ["input"], ["output"])], X.shape[1]), X)["output"]
    want = np.clip(np.float64(np.float32(0.2)) * X.astype(np.float64) + 0.5, 0.0, 1.0)   # the ONNX defaults
    assert float(np.abs(got - want).max()) <= TOL_EXEC
    assert got.min() == 0.0 and got.max() == 1.0   # both clamps are reached on these inputs


@pytest.mark.parametrize("per_column", [False, True])
def test_executor_prelu_matches_torch(per_column):
    import torch.nn.functional as F
    X = _x()
    C = X.shape[1]
    slope = R.affine(C)[0] * 0.2 if per_column else np.array([0.25], np.float32)
    got = _run(_graph([node("PRelu", ["input", "sl"], ["output"])], C, [tensor("sl", slope)]), X)["output"]
    want = F.prelu(_t64(X), _t64(slope)).numpy()
    assert float(np.abs(got - want).max()) <= TOL_EXEC


def test_executor_softplus_is_overflow_safe():
    X = np.array([[-100.0, 100.0, 0.0, 1e4]], np.float32)
    got = _run(_graph([node("Softplus", ["input"], ["output"])], 4), X)["output"]
    np.testing.assert_allclose(got, [[0.0, 100.0, np.log(2.0), 1e4]], rtol=1e-7, atol=1e-30)


@pytest.mark.parametrize("ratio", [False, True])
def test_executor_dropout_is_identity(ratio):
    X = _x()
    ins, inits = (["input", "r"], [tensor("r", np.array(0.5, np.float32))]) if ratio else (["input"], [])
    g = _graph([node("Dropout", ins, ["output"])], X.shape[1], inits)
    np.testing.assert_array_equal(_run(g, X)["output"], X)
    # the mask is produced (all ones) only when something reads it
    g = _graph([node("Dropout", ins, ["d", "mask"]), node("Mul", ["d", "mask"], ["output"])], X.shape[1], inits)
    np.testing.assert_array_equal(_run(g, X)["output"], X)


def test_executor_rejections_name_op_and_cause():
    C = 8
    X = _x(C, 4)
    ones = tensor("o", np.ones(C, np.float32))
    cases = [
        (_graph([node("BatchNormalization", ["input", "o", "o", "o", "o"], ["output"], training_mode=1)], C, [ones]),
         "BatchNormalization: training_mode"),
        (_graph([node("LayerNormalization", ["input", "o"], ["output"], axis=0)], C, [ones]), "LayerNormalization: axis"),
        (_graph([node("LayerNormalization", ["input"], ["output"])], C), "LayerNormalization: Scale"),
        (_graph([node("Dropout", ["input", "", "t"], ["output"])], C, [tensor("t", np.array(True))]),
         "Dropout: training_mode"),
        (_graph([node("Gelu", ["input"], ["output"], approximate="fast")], C), "Gelu: approximate"),
        (_graph([node("PRelu", ["input", "s3"], ["output"])], C, [tensor("s3", np.ones(3, np.float32))]), "PRelu: slope"),
    ]
    for g, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            _run(g, X)


# ------------------------------------------------------------------------------ lowering
ACT = {"none": lambda v: v, "relu": lambda v: np.maximum(v, 0), "sigmoid": lambda v: 1 / (1 + np.exp(-v)),
       "tanh": np.tanh}


def run_plan_numpy(plan, X):
    """The lowered plan evaluated on the host in float64: what K3 dense / head, join and the row
    ops compute."""
    vals = []

    def val(k):
        return X.astype(np.float64) if k < 0 else vals[k]
    for i, s in enumerate(plan.steps):
        if s.kind == "join":
            a, b = val(s.a)[:, :s.na], val(s.b)[:, :s.nb]
            y = a + b if s.op == "add" else np.concatenate([a, b], 1)
        else:
            x = val(step_inputs(plan.steps, i)[0])
            if s.kind == "dense":
                y = ACT[s.act](x[:, :s.k] @ s.w_np.T.astype(np.float64) + (0 if s.b_np is None else s.b_np))
            elif s.kind == "head":
                h = ACT[s.act1](x[:, :s.k] @ s.w1_np.T.astype(np.float64) + (0 if s.b1_np is None else s.b1_np))
                y = ACT[s.act2](h @ s.w2_np + s.b2)[:, None]
            elif s.kind == "row" and s.op == "layernorm":
                y = R.ref_layernorm(x[:, :s.width], s.gamma_np, s.beta_np, s.eps)
            elif s.kind == "row" and s.op == "softmax":
                y = R.ref_softmax(x[:, :s.width])
            elif s.kind == "row":
                y = R.ref_act(s.act, x[:, :s.width], s.p0, s.p1, s.gamma_np)
            else:
                raise AssertionError(s.kind)
        vals.append(y)
    return vals[-1]


def _check_plan(m, width, kinds=None, rows=257):
    om = _load(m)
    plan = compile_onnx(om)
    if kinds is not None:
        assert [s.kind for s in plan.steps] == kinds, plan.describe()
    X = np.random.default_rng(5).standard_normal((rows, width)).astype(np.float32)
    ref = np.asarray(N.Executor(om).run({"input": X})[plan.output_name]).reshape(rows, -1)
    got = run_plan_numpy(plan, X)
    np.testing.assert_allclose(got[:, plan.ml_col], ref[:, plan.executor_col], atol=1e-5, rtol=1e-5)
    assert executor_output(om) == (plan.executor_col, plan.output_name)
    return plan


@pytest.mark.parametrize("kind,kw,kinds", R.MODEL_CASES, ids=[R.model_id(c) for c in R.MODEL_CASES])
def test_builders_lower_and_match_executor(kind, kw, kinds):
    """BatchNormalization and Dropout add no step; the activations the dense epilogue lacks and
    the Relu after a residual Add run as row steps; the plan computes what the executor does."""
    m = builders.build(kind, **kw)
    plan = _check_plan(m, kw["n_features"], kinds)
    ops = [n.op_type for n in m.graph.node]
    steps = plan.steps
    assert "Dropout" in ops and ("BatchNormalization" in ops or "LayerNormalization" in ops)
    if kind == "torch_mlp":
        # one dense layer per Gemm at the most: the BatchNormalization folded into it
        assert sum(s.kind in ("dense", "head") for s in steps) <= ops.count("Gemm")
        if kw["out"] == 2:   # the two-logit Softmax: one sigmoid column, the executor's column 1
            assert plan.out_width == 1 and plan.ml_col == 0 and plan.executor_col == 1
        if kw["act"] == "LeakyRelu":   # a row step behind every hidden dense layer
            rows = [i for i, s in enumerate(steps) if s.kind == "row"]
            assert len(rows) == kw["layers"] and all(steps[i - 1].kind == "dense" and steps[i].act == "leaky_relu"
                                                    for i in rows)
        else:
            assert all(s.kind != "row" for s in steps)
    else:
        joins = [i for i, s in enumerate(steps) if s.kind == "join"]
        assert len(joins) == kw["blocks"] and not plan.is_chain
        assert all(steps[i + 1].kind == "row" and steps[i + 1].act == "relu" for i in joins)   # Relu(Add(skip))
        assert sum(s.kind == "row" and s.op == "layernorm" for s in steps) == (kw["blocks"] + 1) * (kw["norm"] == "layer")


def test_two_logit_relu_mlp_runs_on_the_fused_head():
    """Gemm -> BatchNormalization -> Relu -> Dropout [x layers] -> Gemm(.., 2) -> Softmax: the
    last hidden layer and the narrowed logit layer fuse into the head. With one Gemm in front of
    the logits that head is the whole plan; with two the plan is dense -> head."""
    for layers, kinds in ((1, ["head"]), (2, ["dense", "head"])):
        plan = compile_onnx(_load(builders.torch_mlp(n_features=30, hidden=64, layers=layers, act="Relu", out=2)))
        assert [s.kind for s in plan.steps] == kinds, plan.describe()
        assert plan.ml_col == 0 and plan.executor_col == 1 and plan.out_width == 1
        assert plan.steps[-1].act1 == "relu" and plan.steps[-1].act2 == "sigmoid"


OTHER_ACTS = [("Elu", dict(alpha=0.7), "elu"), ("Selu", {}, "selu"), ("Softplus", {}, "softplus"),
              ("HardSigmoid", {}, "hard_sigmoid"), ("Gelu", {}, "gelu"), ("Gelu", dict(approximate="tanh"), "gelu_tanh"),
              ("Clip", dict(min=-0.5, max=0.75), "clip"), ("PRelu", {}, "prelu"), ("LeakyRelu", dict(alpha=0.2), "leaky_relu")]


@pytest.mark.parametrize("op,attrs,act", OTHER_ACTS, ids=[c[2] for c in OTHER_ACTS])
def test_activation_lowers_to_a_row_step(op, attrs, act):
    rng = np.random.default_rng(8)
    w1, w2 = rng.standard_normal((12, 20)).astype(np.float32) * 0.4, rng.standard_normal((20, 1)).astype(np.float32) * 0.4
    inits = [tensor("W1", w1), tensor("W2", w2), tensor("sl", rng.uniform(0.05, 0.4, 20).astype(np.float32))]
    ins = ["h", "sl"] if op == "PRelu" else ["h"]
    g = _graph([node("MatMul", ["input", "W1"], ["h"]), node(op, ins, ["a"], **attrs), node("MatMul", ["a", "W2"], ["o"]),
                node("Sigmoid", ["o"], ["output"])], 12, inits, out_width=1)
    plan = _check_plan(g, 12, ["dense", "row", "dense"])
    assert plan.steps[1].op == "act" and plan.steps[1].act == act and plan.steps[1].width == 20
    assert "row" not in plan.describe() and act in plan.describe()


def test_softmax_wide_and_shared_logits_run_as_row_steps():
    rng = np.random.default_rng(9)
    for n_out, col in ((2, 1), (5, 0)):
        w = rng.standard_normal((12, n_out)).astype(np.float32)
        # the logits have a second reader (n_out 2) / are wider than two: no narrowing
        nodes = [node("MatMul", ["input", "W"], ["z"]), node("Softmax", ["z"], ["p"], axis=-1)]
        nodes += ([node("Mul", ["z", "zero"], ["z0"]), node("Add", ["p", "z0"], ["output"])] if n_out == 2
                  else [node("Identity", ["p"], ["output"])])
        g = _graph(nodes, 12, [tensor("W", w), tensor("zero", np.zeros(1, np.float32))], out_width=n_out)
        plan = compile_onnx(_load(g))
        assert [s.kind for s in plan.steps][:2] == ["dense", "row"] and plan.steps[1].op == "softmax"
        if n_out == 5:
            assert (plan.ml_col, plan.executor_col) == (col, col)
        X = rng.standard_normal((33, 12)).astype(np.float32)
        ref = np.asarray(N.Executor(_load(g)).run({"input": X})["output"])
        np.testing.assert_allclose(run_plan_numpy(plan, X), ref, atol=1e-5, rtol=1e-5)
    # two columns straight from a Softmax row step: the positive class is column 1 on both sides
    g = _graph([node("Relu", ["input"], ["r"]), node("Softmax", ["r"], ["output"])], 2)
    plan = _check_plan(g, 2, ["row", "row"])
    assert (plan.ml_col, plan.executor_col) == (1, 1)


def test_clip_at_zero_is_a_relu_and_folds():
    w = np.random.default_rng(10).standard_normal((12, 16)).astype(np.float32)
    g = _graph([node("MatMul", ["input", "W"], ["h"]), node("Clip", ["h", "lo"], ["output"])], 12,
               [tensor("W", w), tensor("lo", np.zeros((), np.float32))], out_width=16)
    plan = _check_plan(g, 12, ["dense"])
    assert plan.steps[0].act == "relu"


def test_activations_that_cannot_fold_become_row_steps():
    """Relu / Sigmoid / Tanh still fold into a dense epilogue; after another activation, or on a
    value with a second reader, they run as a row step (they raised before)."""
    rng = np.random.default_rng(11)
    w = rng.standard_normal((12, 12)).astype(np.float32) * 0.3
    g = _graph([node("MatMul", ["input", "W"], ["h"]), node("Relu", ["h"], ["r"]), node("Tanh", ["r"], ["t"]),
                node("Sigmoid", ["h"], ["s"]), node("Add", ["t", "s"], ["output"])], 12, [tensor("W", w)])
    plan = _check_plan(g, 12)
    # h has two readers (Relu, Sigmoid): neither folds; Tanh follows an activation
    assert [s.kind for s in plan.steps] == ["dense", "row", "row", "row", "join"], plan.describe()
    assert plan.steps[0].act == "none" and sorted(s.act for s in plan.steps[1:4]) == ["relu", "sigmoid", "tanh"]


def test_layer_norm_applies_a_pending_affine_first():
    C = 16
    gam, bet = R.affine(C)
    sc = np.random.default_rng(12).uniform(0.5, 2.0, C).astype(np.float32)
    g = _graph([node("Mul", ["input", "sc"], ["x"]), node("LayerNormalization", ["x", "g", "b"], ["output"], epsilon=1e-3)],
               C, [tensor("sc", sc), tensor("g", gam), tensor("b", bet)])
    plan = _check_plan(g, C, ["dense", "row"])
    assert plan.steps[1].eps == pytest.approx(1e-3) and "layernorm(16)" in plan.describe()


# ------------------------------------------------------------------------------ refusals
def _refusals():
    C = 8
    ones, W = tensor("o", np.ones(C, np.float32)), tensor("W", np.eye(C, dtype=np.float32))
    w1 = tensor("w1", np.ones((C, 1), np.float32))
    lstm = builders.build("lstm", seq=4, in_dim=C, hidden=C, layers=1, head=False)
    seq_nodes = [n for n in lstm.graph.node]
    seq_nodes[-1].output[0] = "hs"
    seq = model(seq_nodes + [node("LayerNormalization", ["hs", "o"], ["output"])],
                list(lstm.graph.input), [value_info("output", S.FLOAT, ["N", C])], list(lstm.graph.initializer) + [ones])
    return [
        ("bn-training", _graph([node("BatchNormalization", ["input", "o", "o", "o", "o"], ["output"], training_mode=1)],
                               C, [ones]), "BatchNormalization: training_mode"),
        ("ln-axis", _graph([node("LayerNormalization", ["input", "o"], ["output"], axis=0)], C, [ones]),
         "LayerNormalization: axis 0"),
        ("ln-mean-read", _graph([node("LayerNormalization", ["input", "o"], ["y", "mean"]),
                                 node("Sub", ["y", "mean"], ["output"])], C, [ones]), "Mean / InvStdDev"),
        ("softmax-axis0", _graph([node("Softmax", ["input"], ["output"], axis=0)], C), "Softmax: axis 0"),
        ("dropout-mask-read", _graph([node("Dropout", ["input"], ["d", "mask"]), node("Mul", ["d", "mask"], ["output"])], C),
         "Dropout: its mask"),
        ("prelu-slope", _graph([node("MatMul", ["input", "W"], ["h"]), node("Sigmoid", ["h"], ["sl"]),
                                node("PRelu", ["input", "sl"], ["output"])], C, [W]), "PRelu: the slope must be a constant"),
        ("clip-bounds", _graph([node("MatMul", ["input", "w1"], ["h"]), node("Sigmoid", ["h"], ["hi"]),
                                node("Clip", ["input", "", "hi"], ["output"])], C, [w1]), "Clip: max must be a constant"),
        ("row-in-sequence", seq, "row step .* sequence plan"),
    ]


@pytest.mark.parametrize("name,m,msg", _refusals(), ids=[c[0] for c in _refusals()])
def test_plan_refusals_name_the_cause(name, m, msg):
    with pytest.raises(PlanError, match=msg):
        compile_onnx(_load(m))


# ------------------------------------------------------------------------------ engine
def test_engine_cpu_scores_a_torch_mlp_with_the_positive_class():
    """RiskEngine(backend="cpu") with the two-logit torch_mlp as the fraud model: ml_score is the
    executor's column 1 on the rows an independent golden store assembles for the same traffic."""
    from igaming_platform_amd.config import TX_TYPE_ID, Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.golden.features import GoldenFeatureStore, model_input
    from igaming_platform_amd.utils.hashing import SEED_IP, id_hash
    from tests.test_engine_cpu import NOW, _txs
    m = builders.torch_mlp(n_features=30, out=2)
    cfg = Config()
    eng = RiskEngine(cfg, backend="cpu", capacity=64, fraud_model=m.SerializeToString())
    txs = _txs(60, np.random.default_rng(7))
    got = np.array([r["ml_score"] for r in eng.score(txs, now=NOW)], np.float64)
    eng.close()
    st = GoldenFeatureStore(cfg.features)   # every row is scored on the state before the batch
    X = np.stack([model_input(st.raw_features(t["account_id"], NOW, ip_hash=id_hash(t["ip_address"], SEED_IP)),
                              t["amount"], TX_TYPE_ID[t["transaction_type"]], cfg.features.log_transform, 30)
                  for t in txs]).astype(np.float32)
    ref = np.asarray(_run(m, X)["output"])[:, 1]
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
    assert np.all((got > 0) & (got < 1)) and np.ptp(got) > 1e-3
