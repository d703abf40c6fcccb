"""Per-sequence lengths (ONNX sequence_lens) without a GPU: the C++ executor against the per-row
float64 reference of tests/seqlen_cases.py, the plan compiler, the builders, the alignment identity
the CPU twins and the kernels rest on, the conditions on the tolerances of tests/test_seqlen_gpu.py,
and the CPU abuse paths on a masked model.

Tolerance conditions, measured on the references alone (test_tolerances_come_from_the_reference):
the GPU comparisons use gru_cases.YH_TOL / OUT_TOL / SPLIT_TOL and lstm_cases.tol(name) / SPLIT_TOL
as they stand. Over the bf16 cases of seqlen_cases.CASES the float32-vs-float64 gap of the
bf16-emulating reference is at most 1.90e-5 in yh (gru-D, gru-D-32) and 1.39e-4 in out (lstm-E-32);
4x these stay below every shared bound (the smallest: lstm yh 1.87e-4, gru out 1.9e-3), so no case
has a bound of its own.

Discrimination (test_short_rows_tell_masked_from_zero_padded): over every row with len < T of every
case, the masked reference and the unmasked reference on the right-aligned zero-padded input (what the
kernels computed before they honoured lengths) differ in yh by at least 1.68x four times the case's yh
bound (gru-D and gru-E-unpiped-32, rows of length T - 1; 3.09e-3 against 1.84e-3). The X seeds are
the table models' seeds + 2000; no other seed had to be tried."""
import hashlib

import numpy as np
import pytest

from igaming_platform_amd.native import native
from igaming_platform_amd.onnx import builders
from igaming_platform_amd.onnx import schema as S
from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
from tests import gru_cases as G
from tests import lstm_cases as L
from tests import seqlen_cases as Q

EXECUTOR_TOL = L.EXECUTOR_TOL  # 2e-6, the bound test_gru_edges.py uses for the GRU as well
ROWS, T, H, I = 11, 7, 16, 8


def _load(b):
    return native().OnnxModel.from_bytes(b if isinstance(b, bytes) else b.SerializeToString())


# ------------------------------------------------------------------------------ dispatch coverage
def test_table_reaches_every_masked_instance():
    """Every case resolves, through the dispatch mirrors of the edge suites, to the instance written
    beside it; the table reaches every entry of REQUIRED; no masked case resolves to a cluster kernel
    (E is the cluster shape: a masked launch passes ws = 0 whatever the caller asks)."""
    for c in Q.CASES:
        assert Q.dispatch(c) == c.inst, c.id
        assert "ws" not in Q.instance(c)[0]
    reached = {Q.instance(c) for c in Q.CASES}
    assert reached == set(Q.REQUIRED)
    assert len(Q.REQUIRED) == len(set(Q.REQUIRED)) == 25
    assert {c.reverse for c in Q.CASES if c.kind == "gru"} == {False, True}
    assert {c.reverse for c in Q.CASES if c.kind == "lstm"} == {False, True}
    assert {c.T for c in Q.CASES} == {1, 2, 3, 7}


def test_lens_differ_inside_every_group_and_tile():
    for c in Q.CASES:
        lens = Q.case_lens(c)[:Q.ROWS]
        assert lens.min() >= 0 and lens.max() <= c.T
        if c.T < 7:
            continue
        for g in range(0, Q.ROWS - 3, 4):
            assert len(set(lens[g:g + 4])) > 1, (c.id, g)
        for t0 in (0, 32):   # the first and the last 16-row tile hold both extremes
            assert {0, c.T} <= set(lens[t0:t0 + 15]), (c.id, t0)


# ------------------------------------------------------------------------------ tolerance conditions
def test_tolerances_come_from_the_reference():
    worst = [0.0, 0.0]
    for c in Q.CASES:
        if c.split:
            continue
        y64, o64 = Q.reference(c.id)
        y32, o32 = Q.reference(c.id, "float32")
        gy, go = float(np.abs(y64 - y32).max()), float(np.abs(o64 - o32).max())
        yt, ot = Q.tol(c)
        print(f"{c.id}: f32-vs-f64 gap of the bf16 reference yh {gy:.2e} out {go:.2e}; bounds {yt:.2e} / {ot:.2e}")
        worst = [max(worst[0], gy), max(worst[1], go)]
        assert 4 * gy <= yt and 4 * go <= ot, c.id
    print(f"largest gaps: yh {worst[0]:.2e} out {worst[1]:.2e}")


def test_short_rows_tell_masked_from_zero_padded():
    smallest = None
    for c in Q.CASES:
        layers, head = Q.weights(c)
        X, lens = Q.case_x(c.id), Q.case_lens(c)
        ym, _ = Q.reference(c.id)
        yu, _ = Q.unmasked_ref(c.kind, layers, head, Q.right_align(X, lens), c.reverse, not c.split)
        short = np.flatnonzero(lens < c.T)
        assert len(short)
        d = np.abs(ym - yu).max(axis=1)[short]
        margin = float(d.min() / (4 * Q.tol(c)[0]))
        print(f"{c.id}: smallest yh difference {d.min():.2e} (len {lens[short][d.argmin()]}), margin {margin:.2f}")
        assert margin > 1.0, c.id
        smallest = margin if smallest is None else min(smallest, margin)
    print(f"smallest margin {smallest:.2f}")


# ------------------------------------------------------------------------------ executor
def _layer(rng, kind, D):
    g = 3 if kind == "gru" else 4
    return (rng.uniform(-0.5, 0.5, (D, g * H, I)).astype(np.float32), rng.uniform(-0.5, 0.5, (D, g * H, H)).astype(np.float32),
            rng.uniform(-0.5, 0.5, (D, 2 * g * H)).astype(np.float32))


def _node_model(kind, direction, layout, lens_type=S.INT32, lens_init=None, seed=3):
    """One GRU / LSTM node with sequence_lens wired (a graph input, or the initializer ``lens_init``);
    graph outputs Y and Y_h. Returns (model bytes, (W, R, B) with the direction axis)."""
    D = 2 if direction == "bidirectional" else 1
    W, R, B = _layer(np.random.default_rng(seed), kind, D)
    attrs = dict(hidden_size=H, direction=direction)
    if kind == "gru":
        attrs["linear_before_reset"] = 1
    if layout:
        attrs["layout"] = 1
    n = node(kind.upper(), ["input", "W", "R", "B", "lens"], ["Y", "Yh"], **attrs)
    ins = [value_info("input", S.FLOAT, ["N", T, I] if layout else [T, "N", I])]
    inits = [tensor("W", W), tensor("R", R), tensor("B", B)]
    if lens_init is None:
        ins.append(value_info("lens", lens_type, ["N"]))
    else:
        inits.append(tensor("lens", lens_init))
    outs = [value_info("Y", S.FLOAT, ["N", T, D, H] if layout else [T, D, "N", H]),
            value_info("Yh", S.FLOAT, ["N", D, H] if layout else [D, "N", H])]
    return model([n], ins, outs, inits, name="seqlen_node").SerializeToString(), (W, R, B)


def _ref_layers(kind, W, R, B, d):
    return [(W[d], R[d], B[d], 1)] if kind == "gru" else [(W[d], R[d], B[d])]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("direction", ["forward", "reverse", "bidirectional"])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_executor_matches_the_per_row_reference(kind, direction, layout):
    """Y_h against masked_ref at 2e-6, in every direction and layout; Y is zero past each row's length
    and its last live step equals Y_h (forward: step len - 1; reverse: step 0)."""
    mb, (W, R, B) = _node_model(kind, direction, layout)
    X = np.random.default_rng(17).standard_normal((T, ROWS, I)).astype(np.float32)
    lens = Q.lens_for(ROWS, T, 3)
    feed = np.ascontiguousarray(X.transpose(1, 0, 2)) if layout else X
    out = native().Executor(_load(mb)).run({"input": feed, "lens": lens})
    Y, Yh = out["Y"], out["Yh"]
    if layout:  # [N, T, D, H] -> [T, D, N, H]; [N, D, H] -> [D, N, H]
        Y, Yh = Y.transpose(1, 2, 0, 3), Yh.transpose(1, 0, 2)
    dirs = [False, True] if direction == "bidirectional" else [direction == "reverse"]
    for d, rev in enumerate(dirs):
        ref, _ = Q.masked_ref(kind, _ref_layers(kind, W, R, B, d), None, X, lens, rev, False)
        gap = float(np.abs(Yh[d] - ref).max())
        print(f"{kind} {direction} layout {layout} dir {d}: Y_h gap {gap:.2e}")
        assert gap <= EXECUTOR_TOL
        for b, n in enumerate(lens):
            assert not Y[n:, d, b].any(), f"row {b}: Y is not zero past its length {n}"
            if n:
                assert np.array_equal(Y[0 if rev else n - 1, d, b], Yh[d, b])
            else:
                assert not Yh[d, b].any()


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_executor_refuses_bad_lens(kind):
    X = np.zeros((T, 3, I), np.float32)
    ex = native().Executor(_load(_node_model(kind, "forward", 0)[0]))
    ex.run({"input": X, "lens": np.array([0, T, 3], np.int32)})
    for bad in (np.array([1, 2, 3], np.int64), np.array([1, T + 1, 3], np.int32), np.array([1, -1, 3], np.int32),
                np.array([1, 2], np.int32)):
        with pytest.raises(RuntimeError, match="sequence_lens"):
            ex.run({"input": X, "lens": bad})
    ex64 = native().Executor(_load(_node_model(kind, "forward", 0, lens_init=np.full(3, 6, np.int64))[0]))
    with pytest.raises(RuntimeError, match="sequence_lens"):
        ex64.run({"input": X})


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_alignment_identity(kind, reverse):
    """What the CPU twins and the kernels rest on: with a zero initial state, left-aligned X with lens
    gives each row the Y_h of its own history alone - the right-aligned zero-padded history with the
    padding cut off, run unmasked at T = len. Exact: the same float operations in the same order."""
    mb, _ = _node_model(kind, "reverse" if reverse else "forward", 0)
    ex = native().Executor(_load(mb))
    lens = Q.lens_for(ROWS, T, 5)
    Xr = Q.right_align(np.random.default_rng(23).standard_normal((T, ROWS, I)).astype(np.float32), lens)
    Yh = ex.run({"input": Q.left_align(Xr, lens), "lens": lens})["Yh"][0]
    for b, n in enumerate(lens):
        if n == 0:
            assert not Yh[b].any()
            continue
        cut = np.ascontiguousarray(Xr[T - n:, b:b + 1])          # the padding cut off: T = n, full length
        mb_n = _node_model_T(kind, reverse, int(n))
        alone = native().Executor(_load(mb_n)).run({"input": cut})["Yh"][0, 0]
        assert np.array_equal(Yh[b], alone), f"row {b} len {n}"
    # and the padding matters: the unmasked run over the padded window differs on the short rows
    padded = ex.run({"input": Xr, "lens": np.full(ROWS, T, np.int32)})["Yh"][0]
    short = lens < T
    assert float(np.abs(padded - Yh)[short].max(axis=1).min()) > 1e-3


def _node_model_T(kind, reverse, Tn, seed=3):
    """_node_model's node without sequence_lens at sequence length ``Tn`` (same weights)."""
    W, R, B = _layer(np.random.default_rng(seed), kind, 1)
    attrs = dict(hidden_size=H, direction="reverse" if reverse else "forward")
    if kind == "gru":
        attrs["linear_before_reset"] = 1
    n = node(kind.upper(), ["input", "W", "R", "B"], ["Y", "Yh"], **attrs)
    return model([n], [value_info("input", S.FLOAT, [Tn, "N", I])], [value_info("Yh", S.FLOAT, [1, "N", H])],
                 [tensor("W", W), tensor("R", R), tensor("B", B)], name="seqlen_node_T").SerializeToString()


# ------------------------------------------------------------------------------ plan and builders
# sha256 of the serialized builder output without seq_lens, computed on the commit before this feature
PARENT_SHA = {
    "gru": "6978895118eafd672d43dd29d96848229912dacd704fa3778b55f6e9748607ac",
    "lstm": "b2987b5c133c656cec5183c4c555f0141d881fa93502cbfc62f3461c013b9d0d",
    "gru_bi": "4e38958e9f8729dea9b202e9e488f65a55b9ce5f1ff02a171e447086cf64425f",
    "lstm_rev": "ab1ce17b0138cef4e5557942aaec24c7ad62e24c316890b38a80f195370ecd93",
}


def test_builders_without_seq_lens_are_byte_equal_to_before():
    got = {
        "gru": builders.gru(seq=7, in_dim=16, hidden=64),
        "lstm": builders.lstm(seq=7, in_dim=16, hidden=64),
        "gru_bi": builders.gru(seq=7, in_dim=16, hidden=64, layers=1, direction="bidirectional", layout=1),
        "lstm_rev": builders.lstm(seq=7, in_dim=8, hidden=64, layers=1, direction="reverse", head=False),
    }
    for k, m in got.items():
        assert hashlib.sha256(m.SerializeToString()).hexdigest() == PARENT_SHA[k], k


@pytest.mark.parametrize("kw", [dict(layers=2), dict(layers=1, direction="bidirectional"),
                                dict(layers=1, direction="reverse", layout=1)])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_plan_lowers_builder_models_with_seq_lens(kind, kw):
    from igaming_platform_amd.models.plan import compile_onnx
    build = getattr(builders, kind)
    m = _load(build(seq=7, in_dim=16, hidden=64, seq_lens=True, **kw))
    assert [v[0] for v in m.inputs()] == ["input", "sequence_lens"]
    plan = compile_onnx(m)
    rec = [s for s in plan.steps if s.kind == kind]
    assert len(rec) == kw["layers"] and all(s.masked for s in rec)
    assert plan.lens_input == "sequence_lens" and plan.input_name == "input"
    assert f"{kind}(I=16,H=64,lens)" in plan.describe()
    if rec[0].bidirectional:
        assert rec[0].direction(0).masked and rec[0].direction(1).masked
    plain = compile_onnx(_load(build(seq=7, in_dim=16, hidden=64, **kw)))
    assert plain.lens_input is None and not any(getattr(s, "masked", False) for s in plain.steps)
    assert ",lens" not in plain.describe()


def _two_layer(kind, lens0, lens1, extra_inputs=(), inits=()):
    g = 3 if kind == "gru" else 4
    rng = np.random.default_rng(1)
    w = lambda *s: rng.uniform(-0.3, 0.3, s).astype(np.float32)  # noqa: E731
    op = kind.upper()
    nodes = [node(op, ["input", "W1", "R1", "B1"] + ([lens0] if lens0 else []), ["Y1", "Yh1"], hidden_size=64),
             node("Squeeze", ["Y1", "ax1"], ["X2"]),
             node(op, ["X2", "W2", "R2", "B2"] + ([lens1] if lens1 else []), ["Y2", "Yh2"], hidden_size=64),
             node("Reshape", ["Yh2", "shp"], ["output"])]
    ins = [value_info("input", S.FLOAT, [7, "N", 16])] + list(extra_inputs)
    ii = [tensor("W1", w(1, g * 64, 16)), tensor("R1", w(1, g * 64, 64)), tensor("B1", w(1, 2 * g * 64)),
          tensor("W2", w(1, g * 64, 64)), tensor("R2", w(1, g * 64, 64)), tensor("B2", w(1, 2 * g * 64)),
          tensor("ax1", np.array([1], np.int64)), tensor("shp", np.array([-1, 64], np.int64))] + list(inits)
    return _load(model(nodes, ins, [value_info("output", S.FLOAT, ["N", 64])], ii, name="two"))


@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_plan_refuses_what_it_cannot_mask(kind):
    from igaming_platform_amd.models.plan import PlanError, compile_onnx
    la, lb = value_info("la", S.INT32, ["N"]), value_info("lb", S.INT32, ["N"])
    assert compile_onnx(_two_layer(kind, "la", "la", [la])).lens_input == "la"
    with pytest.raises(PlanError, match="sequence_lens"):   # layers with different lens inputs
        compile_onnx(_two_layer(kind, "la", "lb", [la, lb]))
    with pytest.raises(PlanError, match="sequence_lens"):   # only one of the layers reads it
        compile_onnx(_two_layer(kind, "la", None, [la]))
    with pytest.raises(PlanError, match="sequence_lens"):   # an initializer, even an int32 one
        compile_onnx(_two_layer(kind, "la", "la", inits=[tensor("la", np.full(3, 6, np.int32))]))
    with pytest.raises(PlanError, match="sequence_lens"):   # not int32
        compile_onnx(_two_layer(kind, "la", "la", [value_info("la", S.INT64, ["N"])]))
    with pytest.raises(PlanError, match="sequence_lens"):   # not [N]
        compile_onnx(_two_layer(kind, "la", "la", [value_info("la", S.INT32, ["N", 1])]))
    with pytest.raises(PlanError):                            # any other extra graph input is still refused
        compile_onnx(_extra_input_model(kind))


def _extra_input_model(kind):
    """A GRU / LSTM whose initial_h is a second graph input: not the lens exemption."""
    g = 3 if kind == "gru" else 4
    rng = np.random.default_rng(2)
    w = lambda *s: rng.uniform(-0.3, 0.3, s).astype(np.float32)  # noqa: E731
    nodes = [node(kind.upper(), ["input", "W", "R", "B", "", "h0"], ["Y", "Yh"], hidden_size=64),
             node("Reshape", ["Yh", "shp"], ["output"])]
    return _load(model(nodes, [value_info("input", S.FLOAT, [7, "N", 16]), value_info("h0", S.FLOAT, [1, "N", 64])],
                       [value_info("output", S.FLOAT, ["N", 64])],
                       [tensor("W", w(1, g * 64, 16)), tensor("R", w(1, g * 64, 64)), tensor("B", w(1, 2 * g * 64)),
                        tensor("shp", np.array([-1, 64], np.int64))], name="extra"))


def test_masked_ref_is_the_unmasked_reference_at_full_length():
    """lens = T everywhere: masked_ref equals the edge suites' references row for row (to rounding of
    the batched matrix products), so the new reference adds no recurrence of its own."""
    for c in (Q.BY_ID["pipe-E"], Q.BY_ID["lstm-E"]):
        layers, head = Q.weights(c)
        X = Q.case_x(c.id)[:, :5]
        ym, om = Q.masked_ref(c.kind, layers, head, X, np.full(5, c.T), c.reverse, True)
        yu, ou = Q.unmasked_ref(c.kind, layers, head, X, c.reverse, True)
        assert float(np.abs(ym - yu).max()) <= 1e-12 and float(np.abs(om - ou).max()) <= 1e-12
    assert G.YH_TOL == 4.6e-4 and G.OUT_TOL == 1.9e-3 and G.SPLIT_TOL == 1e-4 and L.SPLIT_TOL == 1e-4


# ------------------------------------------------------------------------------ CPU abuse paths
NOW = 1_700_000_000
SVC_RING, SVC_T = 12, 7
# (account, events): none, 1, 3, ring - 1 and ring events (the model's window holds the newest 7)
SVC_ACCOUNTS = [("quiet", 0), ("one", 1), ("three", 3), ("almost", SVC_RING - 1), ("full", SVC_RING)]


def svc_model(seq_lens=True):
    """A cfg5-shaped abuse model (two GRU layers, linear_before_reset, N = 1 head) at H = 64, T = 7."""
    return builders.gru(seq=SVC_T, in_dim=16, hidden=64, layers=2, seq_lens=seq_lens).SerializeToString()


def svc_events():
    return [dict(account_id=a, amount=1000 + 7919 * i, transaction_type=("deposit", "bet", "win")[i % 3],
                 ts=NOW - 400 + 13 * i) for a, n in SVC_ACCOUNTS for i in range(n)]


def svc_engine(backend, model):
    """A one-shard engine on a 12-entry event ring holding SVC_ACCOUNTS; returns (engine, ids + an unknown id)."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.layouts import ACCTBATCH
    cfg = Config()
    cfg.features.event_ring = SVC_RING
    cfg.gpu.buckets = [64]
    cfg.gpu.max_batch = 64
    eng = RiskEngine(cfg, backend=backend, capacity=64, abuse_model=model)
    rows = np.zeros(1, ACCTBATCH)
    rows["present"] = 1
    eng.load_batch_features(["quiet"], rows)
    eng.ingest_events(svc_events())
    return eng, [a for a, _ in SVC_ACCOUNTS] + ["nobody"]


def svc_expected():
    """The executor's score of each account's left-aligned history (golden encoding of the same events,
    rounded to the rings' bf16), and the scores of the same weights without sequence_lens on the
    zero-padded histories."""
    import torch
    from igaming_platform_amd.config import TX_TYPE_ID, Config
    from igaming_platform_amd.engine.abuse import left_align_history
    from igaming_platform_amd.golden.features import GoldenFeatureStore, TxEvent
    cfg = Config()
    cfg.features.event_ring = SVC_RING
    gold = GoldenFeatureStore(cfg.features)
    for e in svc_events():
        gold.apply(TxEvent(e["account_id"], e["amount"], TX_TYPE_ID[e["transaction_type"]], 0, 0, e["ts"]))
    hist = [torch.from_numpy(gold.event_history(a).astype(np.float32)).to(torch.bfloat16).float().numpy()
            for a, _ in SVC_ACCOUNTS]
    assert [gold.event_count(a) for a, _ in SVC_ACCOUNTS] == [n for _, n in SVC_ACCOUNTS]
    pairs = [left_align_history(h, n, SVC_T) for h, (_, n) in zip(hist, SVC_ACCOUNTS)]
    lens = np.array([p[1] for p in pairs], np.int32)
    assert lens.tolist() == [0, 1, 3, SVC_T, SVC_T]
    masked = native().Executor(_load(svc_model())).run(
        {"input": np.stack([p[0] for p in pairs], 1), "sequence_lens": lens})["output"].reshape(-1)
    plain = native().Executor(_load(svc_model(False))).run({"input": np.stack(hist, 1)})["output"].reshape(-1)
    return masked, plain, lens


def test_left_align_history():
    from igaming_platform_amd.engine.abuse import left_align_history
    h = np.zeros((5, 2), np.float32)
    h[3:] = [[1, 2], [3, 4]]
    out, n = left_align_history(h, 2)
    assert n == 2 and out.tolist() == [[1, 2], [3, 4], [0, 0], [0, 0], [0, 0]]
    out, n = left_align_history(h, 2, 1)      # a window shorter than the history keeps the newest
    assert n == 1 and out.tolist() == [[3, 4]]
    out, n = left_align_history(h, 0, 3)
    assert n == 0 and not out.any() and out.shape == (3, 2)


def test_cpu_abuse_paths_score_short_histories_on_their_events_alone():
    """AbuseService.check (executor branch) and the native CpuAbuseDevice on a masked model: each
    account gets the executor's score of its left-aligned history; the two paths agree to 1e-6; the
    same weights loaded without sequence_lens score the short accounts differently."""
    from igaming_platform_amd.proto import risk_v1 as P
    from tests.test_acct import _ask
    want, plain, lens = svc_expected()
    eng, ids = svc_engine("cpu", svc_model())
    assert eng.abuse.lens_input == "sequence_lens" and eng.abuse.window == SVC_T
    res = eng.check_bonus_abuse_batch(ids, now=NOW)
    assert res[-1].model_score is None and not res[-1].is_abuser       # the unknown id
    got = np.array([r.model_score for r in res[:-1]], np.float64)
    print(f"masked model: service {got}, executor on left-aligned histories {want}, unmasked twin {plain}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)
    assert eng.acct is not None and eng.acct.serves(native().RPC_ABUSE)
    reqs = [(native().RPC_ABUSE, P.CheckBonusAbuseRequest(account_id=a, bonus_id="welcome")) for a in ids]
    nat = [P.CheckBonusAbuseResponse.FromString(b) for b, e in _ask(eng.acct.router, reqs, now=NOW) if e is None]
    assert len(nat) == len(ids)
    for r, n in zip(res[:-1], nat):
        assert not r.signals or r.signals == ["SEQUENCE_MODEL"], r.signals   # the score is the model's
        assert abs(n.abuse_score - r.abuse_score) <= 1e-6 and abs(n.abuse_score - r.model_score) <= 1e-6
    eng.close()
    # without sequence_lens: the zero-padded steps move the short accounts, not the full ones
    eng0, _ = svc_engine("cpu", svc_model(False))
    assert eng0.abuse.lens_input is None
    got0 = np.array([r.model_score for r in eng0.check_bonus_abuse_batch(ids, now=NOW)[:-1]], np.float64)
    eng0.close()
    np.testing.assert_allclose(got0, plain, rtol=0, atol=1e-7)
    short = lens < SVC_T
    assert np.all(np.abs(got - got0)[short] > 1e-3), np.abs(got - got0)
