"""ONNX LSTM on the host: the C++ executor against torch.nn.LSTM (float64) and a hand-written
numpy loop, the plan lowering (LSTMStep, PlanError causes) and CheckBonusAbuse on the CPU backend."""
import numpy as np
import pytest

from igaming_platform_amd.models.plan import PlanError, compile_onnx
from igaming_platform_amd.native import native
from igaming_platform_amd.onnx import builders, schema as S
from igaming_platform_amd.onnx.writer import model, node, tensor, value_info

NOW = 1_760_000_000
SEQ, ROWS, IN = 12, 5, 16


def _load(proto):
    return native().OnnxModel.from_bytes(proto.SerializeToString())


def _to_torch_order(a, H):
    """ONNX gate blocks i, o, f, c along axis 0 -> PyTorch's i, f, g (= c), o."""
    i, o, f, c = (a[k * H:(k + 1) * H] for k in range(4))
    return np.concatenate([i, f, c, o], 0)


def _torch_lstm_f64(m, X, layers, H, direction, head):
    """The builder's model through torch.nn.LSTM in float64; X [T, rows, I] -> [rows, ...]."""
    import torch
    D = 2 if direction == "bidirectional" else 1
    x = torch.from_numpy(X).double()
    if direction == "reverse":
        x = x.flip(0)  # a reverse layer is a forward layer over the time-reversed sequence
    hn = None
    for l in range(1, layers + 1):
        W, R, B = (np.asarray(m.initializer(f"{k}{l}"), np.float64) for k in "WRB")
        cell = torch.nn.LSTM(W.shape[2], H, num_layers=1, bidirectional=D == 2).double()
        with torch.no_grad():
            for d, sfx in enumerate(["", "_reverse"][:D]):
                getattr(cell, "weight_ih_l0" + sfx).copy_(torch.from_numpy(_to_torch_order(W[d], H)))
                getattr(cell, "weight_hh_l0" + sfx).copy_(torch.from_numpy(_to_torch_order(R[d], H)))
                getattr(cell, "bias_ih_l0" + sfx).copy_(torch.from_numpy(_to_torch_order(B[d][:4 * H], H)))
                getattr(cell, "bias_hh_l0" + sfx).copy_(torch.from_numpy(_to_torch_order(B[d][4 * H:], H)))
            x, (hn, _) = cell(x)
    y = hn.transpose(0, 1).reshape(X.shape[1], D * H)  # [D, N, H] -> [N, D*H]
    if head:
        wh = torch.from_numpy(np.asarray(m.initializer("Wh"), np.float64))
        bh = torch.from_numpy(np.asarray(m.initializer("Bh"), np.float64))
        y = torch.sigmoid(y @ wh + bh)
    return y.detach().numpy()


CASES = [(layers, H, direction, layout, head)
         for layers in (1, 2) for H in (64, 128) for direction in ("forward", "reverse", "bidirectional")
         for layout in (0, 1) for head in (True, False) if not (direction == "bidirectional" and layers == 2)]


@pytest.mark.parametrize("layers,H,direction,layout,head", CASES)
def test_executor_matches_torch_lstm_f64(layers, H, direction, layout, head):
    m = _load(builders.build("lstm", seq=SEQ, in_dim=IN, hidden=H, layers=layers, head=head, direction=direction,
                             layout=layout))
    X = np.random.default_rng(H + layers).standard_normal((SEQ, ROWS, IN)).astype(np.float32)
    feed = np.ascontiguousarray(X.transpose(1, 0, 2)) if layout else X
    got = native().Executor(m).run({"input": feed})["output"]
    ref = _torch_lstm_f64(m, X, layers, H, direction, head)
    assert got.shape == ref.shape
    err = float(np.abs(got - ref).max())
    print(f"lstm executor vs torch f64: max err {err:.3e}")
    assert err <= 2e-6


def _single(extra_inputs=(), inits=(), outputs=("Y", "Yh", "Yc"), H=8, I=4, seed=0, **attrs):
    """One hand-built LSTM node: inputs X, W, R, B + ``extra_inputs`` (names for sequence_lens,
    initial_h, initial_c, P; "" skips one); graph outputs Y_h and Y_c."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(-0.5, 0.5, (1, 4 * H, I)).astype(np.float32)
    R = rng.uniform(-0.5, 0.5, (1, 4 * H, H)).astype(np.float32)
    B = rng.uniform(-0.5, 0.5, (1, 8 * H)).astype(np.float32)
    n = node("LSTM", ["input", "W", "R", "B", *extra_inputs], list(outputs), hidden_size=H, **attrs)
    outs = [value_info(o, S.FLOAT, [1, "N", H]) for o in outputs[1:] if o]
    proto = model([n], [value_info("input", S.FLOAT, [6, "N", I])], outs,
                  [tensor("W", W), tensor("R", R), tensor("B", B), *inits], name="lstm_one")
    return proto, (W[0].astype(np.float64), R[0].astype(np.float64), B[0].astype(np.float64))


def _numpy_lstm(X, W, R, B, h0=None, c0=None, P=None):
    """The ONNX LSTM equations (gates i, o, f, c; peepholes i, o, f) as a float64 loop."""
    H = R.shape[1]
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    h = np.zeros((X.shape[1], H)) if h0 is None else h0.astype(np.float64)
    c = np.zeros((X.shape[1], H)) if c0 is None else c0.astype(np.float64)
    p = np.zeros(3 * H) if P is None else P.astype(np.float64)
    for t in range(X.shape[0]):
        g = X[t].astype(np.float64) @ W.T + h @ R.T + B[:4 * H] + B[4 * H:]
        i = sg(g[:, :H] + p[:H] * c)
        f = sg(g[:, 2 * H:3 * H] + p[2 * H:] * c)
        c = f * c + i * np.tanh(g[:, 3 * H:])
        o = sg(g[:, H:2 * H] + p[H:2 * H] * c)
        h = o * np.tanh(c)
    return h, c


def test_executor_initial_states_match_numpy_loop():
    rng = np.random.default_rng(5)
    h0 = rng.standard_normal((1, 3, 8)).astype(np.float32)
    c0 = rng.standard_normal((1, 3, 8)).astype(np.float32)
    proto, (W, R, B) = _single(("", "h0", "c0"), [tensor("h0", h0), tensor("c0", c0)])
    X = rng.standard_normal((6, 3, 4)).astype(np.float32)
    out = native().Executor(_load(proto)).run({"input": X})
    h, c = _numpy_lstm(X, W, R, B, h0[0], c0[0])
    assert float(np.abs(out["Yh"][0] - h).max()) <= 2e-6
    assert float(np.abs(out["Yc"][0] - c).max()) <= 2e-6


def test_executor_peepholes_match_numpy_loop():
    rng = np.random.default_rng(6)
    P = rng.uniform(-0.5, 0.5, (1, 24)).astype(np.float32)
    proto, (W, R, B) = _single(("", "", "", "P"), [tensor("P", P)])
    X = rng.standard_normal((6, 3, 4)).astype(np.float32)
    out = native().Executor(_load(proto)).run({"input": X})
    h, c = _numpy_lstm(X, W, R, B, P=P[0])
    assert float(np.abs(out["Yh"][0] - h).max()) <= 2e-6
    assert float(np.abs(out["Yc"][0] - c).max()) <= 2e-6
    h_plain, _ = _numpy_lstm(X, W, R, B)
    assert float(np.abs(h - h_plain).max()) > 1e-3  # the peepholes matter in this case


@pytest.mark.parametrize("extra,inits,attrs,cause", [
    (("lens",), [tensor("lens", np.full(3, 6, np.int64))], {}, "sequence_lens"),
    ((), [], dict(activations=["Relu", "Tanh", "Tanh"]), "activations"),
    ((), [], dict(clip=3.0), "clip"),
    ((), [], dict(input_forget=1), "input_forget"),
])
def test_executor_rejects_unsupported_variants(extra, inits, attrs, cause):
    proto, _ = _single(extra, inits, **attrs)
    X = np.zeros((6, 3, 4), np.float32)
    with pytest.raises(RuntimeError, match=cause):
        native().Executor(_load(proto)).run({"input": X})


def test_executor_accepts_explicit_default_activations():
    proto, (W, R, B) = _single(activations=["Sigmoid", "Tanh", "Tanh"])
    X = np.random.default_rng(7).standard_normal((6, 3, 4)).astype(np.float32)
    out = native().Executor(_load(proto)).run({"input": X})
    assert float(np.abs(out["Yh"][0] - _numpy_lstm(X, W, R, B)[0]).max()) <= 2e-6


# ---------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("kw,kinds,widths", [
    (dict(seq=12, hidden=64, layers=1, head=False), ["lstm"], [64]),
    (dict(seq=16, hidden=128, layers=2, head=True, in_dim=40), ["lstm", "lstm", "dense"], [128, 128, 1]),
    (dict(seq=12, hidden=64, layers=1, head=True, direction="bidirectional"), ["lstm", "dense"], [128, 1]),
    (dict(seq=12, hidden=64, layers=2, head=True, direction="reverse", layout=1), ["lstm", "lstm", "dense"],
     [64, 64, 1]),
])
def test_plan_lowers_builder_models(kw, kinds, widths):
    from igaming_platform_amd.models.plan import has_sequence
    plan = compile_onnx(_load(builders.build("lstm", **kw)))
    assert plan.family == "lstm" and plan.seq_input and has_sequence(plan.steps)
    assert [s.kind for s in plan.steps] == kinds
    assert [s.out_width for s in plan.steps] == widths
    first = plan.steps[0]
    H, I = kw["hidden"], kw.get("in_dim", 16)
    assert (first.hidden, first.in_dim, first.seq) == (H, I, kw["seq"])
    assert first.w_np.shape == (4 * H, I) and first.r_np.shape == (4 * H, H) and first.b_np.shape == (8 * H,)
    assert first.reverse == (kw.get("direction") == "reverse") and first.layout == kw.get("layout", 0)
    assert first.bidirectional == (kw.get("direction") == "bidirectional")
    if first.bidirectional:
        assert first.w_rev_np.shape == (4 * H, I)
        rev = first.direction(1)
        assert rev.reverse and not rev.bidirectional and rev.w_np is first.w_rev_np
        assert not first.direction(0).reverse
    assert plan.describe().startswith(f"lstm(I={I},H={H})")


def _headed(extra=(), inits=(), outputs=("Y", "Yh"), tail=(), **attrs):
    """LSTM (H = 8) -> Reshape -> Gemm -> Sigmoid with one unsupported feature switched on."""
    H, I = 8, 8
    rng = np.random.default_rng(1)
    n = node("LSTM", ["input", "W", "R", "B", *extra], list(outputs), hidden_size=H, **attrs)
    base = [tensor("W", rng.standard_normal((1, 4 * H, I)).astype(np.float32)),
            tensor("R", rng.standard_normal((1, 4 * H, H)).astype(np.float32)),
            tensor("B", rng.standard_normal((1, 8 * H)).astype(np.float32)),
            tensor("shp", np.array([-1, H], np.int64)), tensor("Wh", rng.standard_normal((H, 1)).astype(np.float32)),
            tensor("Bh", np.zeros(1, np.float32))]
    nodes = [n, *tail, node("Reshape", [tail[-1].output[0] if tail else "Yh", "shp"], ["h"]),
             node("Gemm", ["h", "Wh", "Bh"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    return _load(model(nodes, [value_info("input", S.FLOAT, [6, "N", I])],
                       [value_info("output", S.FLOAT, ["N", 1])], [*base, *inits], name="lstm_bad"))


def _state(name):
    return tensor(name, np.zeros((1, 3, 8), np.float32))


@pytest.mark.parametrize("kw,cause", [
    (dict(extra=("lens",), inits=[tensor("lens", np.full(3, 6, np.int64))]), "sequence_lens"),
    (dict(extra=("", "h0"), inits=[_state("h0")]), "initial_h"),
    (dict(extra=("", "", "c0"), inits=[_state("c0")]), "initial_c"),
    (dict(extra=("", "", "", "P"), inits=[tensor("P", np.zeros((1, 24), np.float32))]), "peephole"),
    (dict(activations=["Sigmoid", "Relu", "Tanh"]), "activations"),
    (dict(clip=2.0), "clip"),
    (dict(input_forget=1), "input_forget"),
])
def test_plan_refuses_unsupported_variants(kw, cause):
    with pytest.raises(PlanError, match=cause):
        compile_onnx(_headed(**kw))


def test_plan_accepts_the_plain_hand_built_model():
    plan = compile_onnx(_headed(activations=["Sigmoid", "Tanh", "Tanh"]))
    assert [s.kind for s in plan.steps] == ["lstm", "dense"] and plan.family == "lstm"


def test_plan_refuses_a_consumed_cell_state():
    with pytest.raises(PlanError, match="Y_c"):
        compile_onnx(_headed(outputs=("Y", "Yh", "Yc"), tail=[node("Identity", ["Yc"], ["cell"])]))


def test_plan_refuses_lstm_mixed_with_gru():
    H, I = 8, 8
    rng = np.random.default_rng(2)
    inits = [tensor("W", rng.standard_normal((1, 4 * H, I)).astype(np.float32)),
             tensor("R", rng.standard_normal((1, 4 * H, H)).astype(np.float32)),
             tensor("Wg", rng.standard_normal((1, 3 * H, H)).astype(np.float32)),
             tensor("Rg", rng.standard_normal((1, 3 * H, H)).astype(np.float32)),
             tensor("ax", np.array([1], np.int64)), tensor("shp", np.array([-1, H], np.int64))]
    nodes = [node("LSTM", ["input", "W", "R"], ["Y1", "Yh1"], hidden_size=H),
             node("Squeeze", ["Y1", "ax"], ["X2"]),
             node("GRU", ["X2", "Wg", "Rg"], ["Y2", "Yh2"], hidden_size=H),
             node("Reshape", ["Yh2", "shp"], ["output"])]
    m = _load(model(nodes, [value_info("input", S.FLOAT, [6, "N", I])], [value_info("output", S.FLOAT, ["N", H])],
                    inits, name="mixed"))
    with pytest.raises(PlanError, match="mixed"):
        compile_onnx(m)
    # the executor still runs it: the engine's explicit CPU route
    out = native().Executor(m).run({"input": np.zeros((6, 2, I), np.float32)})["output"]
    assert out.shape == (2, H)


# -------------------------------------------------------------------------------------- engine
def test_bonus_abuse_lstm_model_cpu_matches_executor_on_golden_rows():
    """RiskEngine(backend="cpu") with a 2 x 64 LSTM over the last 16 events: the model score of
    accounts with 0, 5 and 20 events equals the executor run on the rows an independent golden
    store encodes for the same events, rounded to the rings' bf16 (20 > 16: the ring keeps the
    newest 16). Same inputs, same executor: the scores agree to float32 printing (1e-7)."""
    from igaming_platform_amd.config import TX_TYPE_ID, Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.golden.features import GoldenFeatureStore, TxEvent
    from igaming_platform_amd.layouts import ACCTBATCH
    cfg = Config()
    cfg.features.event_ring = 16
    proto = builders.build("lstm", seq=16, hidden=64, layers=2)
    eng = RiskEngine(cfg, backend="cpu", capacity=50, abuse_model=proto.SerializeToString())
    rows = np.zeros(1, ACCTBATCH)
    rows["present"] = 1
    eng.load_batch_features(["quiet"], rows)   # a known account without events
    gold = GoldenFeatureStore(cfg.features)
    evs = []
    for acct, n in (("five", 5), ("twenty", 20)):
        for i in range(n):
            e = dict(account_id=acct, amount=1000 + 7919 * i, transaction_type=("deposit", "bet", "win")[i % 3],
                     ts=NOW - 400 + 13 * i)
            evs.append(e)
            gold.apply(TxEvent(acct, e["amount"], TX_TYPE_ID[e["transaction_type"]], 0, 0, e["ts"]))
    eng.ingest_events(evs)
    ids = ["quiet", "five", "twenty"]
    res = eng.check_bonus_abuse_batch(ids, now=NOW)
    import torch
    X = np.stack([gold.event_history(a) for a in ids], axis=1).astype(np.float32)   # [16, 3, 16]
    X = torch.from_numpy(X).to(torch.bfloat16).float().numpy()  # the event rings hold bf16 values
    assert np.count_nonzero(X[:, 0]) == 0 and np.count_nonzero(X[:, 1].any(axis=1)) == 5
    assert np.all(X[:, 2].any(axis=1))
    ref = native().Executor(_load(proto)).run({"input": X})["output"].reshape(-1)
    got = np.array([r.model_score for r in res], np.float64)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-7)
    assert len(set(np.round(got, 6))) == 3
