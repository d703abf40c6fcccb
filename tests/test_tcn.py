"""Temporal-convolution (Conv1D / TCN) sequence models on the CPU: the executor's Conv, Pad, pooling
and reduction operators, rank-3 Gather / Slice, the tcn builder's three causal spellings, the lowering
to ConvStep / SeqPoolStep with its folds, refusals and limits, malformed models, and the CPU engine.
Reference and cases: tests/tcn_cases.py."""
import os
import re

import numpy as np
import pytest

from igaming_platform_amd.models import plan as P
from igaming_platform_amd.models.plan import PlanError, compile_onnx
from igaming_platform_amd.native import native
from igaming_platform_amd.onnx import builders
from igaming_platform_amd.onnx import schema as S
from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
from tests import tcn_cases as C

NOW = 1_760_000_000


def _load(m):
    return native().OnnxModel.from_bytes(m.SerializeToString())


def _run(m, X):
    return native().Executor(_load(m)).run({"input": np.ascontiguousarray(X, np.float32)})["output"]


def _graph(nodes, inits=(), in_dims=("N", 4, 9), out_rank=3):
    return model(nodes, [value_info("input", S.FLOAT, list(in_dims))], [value_info("output", S.FLOAT, ["N"] * out_rank)],
                 list(inits), name="t")


def _scalar(name, v):
    t = tensor(name, np.asarray([v], np.int64))
    del t.dims[:]
    return t


def eval_plan(plan, X):
    """A temporal-convolution plan evaluated in float64 numpy, step by step, from the ConvStep formula."""
    steps = plan.steps
    x = C.to_nct(X, steps[0].layout).astype(np.float64)
    outs = []
    for i, s in enumerate(steps):
        src = x if P.step_inputs(steps, i)[0] < 0 else outs[P.step_inputs(steps, i)[0]]
        if s.kind == "conv":
            y = C.ref_act(C.ref_conv(src, s.w_np.transpose(0, 2, 1), s.b_np, s.dil, s.pad_left), s.act)
            if s.res is not None:
                y = y + outs[s.res]
            outs.append(C.ref_act(y, s.act_post))
        elif s.kind == "seqpool":
            outs.append(C.ref_pool(src, s.op))
        else:
            y = src @ s.w_np.astype(np.float64).T + (0.0 if s.b_np is None else s.b_np.astype(np.float64))
            outs.append(C.ref_act(y, s.act))
    return outs[-1]


# ------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("style", ["pads", "chomp", "pad_op", "same"])
def test_reference_against_torch_float64(style):
    """ref_conv / ref_tcn equal torch.nn.functional.conv1d in float64 (1e-12: both are float64, the
    summation orders differ) for causal and symmetric padding, every read-out."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    for k, d, T in ((1, 1, 1), (2, 3, 5), (3, 2, 17), (8, 7, 17), (3, 4, 2)):
        x, w, b = rng.standard_normal((3, 5, T)), rng.standard_normal((4, 5, k)), rng.standard_normal(4)
        span = d * (k - 1)
        for pl in {0, span, span // 2}:
            want = F.conv1d(F.pad(torch.from_numpy(x), (pl, span - pl)), torch.from_numpy(w), torch.from_numpy(b), dilation=d)
            assert np.abs(C.ref_conv(x, w, b, d, pl) - want.numpy()).max() < 1e-12
    for ro in ("last", "mean", "max"):
        kw = dict(seq=20, in_dim=5, channels=(6, 7), dilations=(1, 3), readout=ro, causal=style != "same",
                  style="pads" if style == "same" else style)
        m = builders.tcn(**kw)
        X = C.real_input(0, n=4, seq=20, in_dim=5)
        assert np.abs(C.ref_tcn(m, X, **kw) - C.torch_tcn(m, X, torch.float64, **kw)).max() < 1e-12


def test_tolerance_derivation():
    """REAL_TOL is 4 x the float32 reference evaluation's largest error on the real-valued models. The torch
    conv1d figure it was recorded from depends on the host's summation order (printed, not asserted); the
    constant is checked against a float32 evaluation in a fixed order, the same on every host: within a
    factor of 2 either way. The executor's own error, deterministic too, stays within a quarter of it."""
    e, s, x = C.f32_error(), C.fixed_order_f32_error(), C.executor_error()
    print(f"float32 evaluation vs float64: torch conv1d on this host {e:.3e}, fixed order {s:.3e} (4 x = {4 * s:.3e}); "
          f"REAL_TOL {C.REAL_TOL:.1e}; executor {x:.3e}")
    assert C.REAL_TOL / 2 <= 4 * s <= C.REAL_TOL * 2
    assert x <= C.REAL_TOL / 4


# ------------------------------------------------------------------------------ executor operators
def _conv_model(w, b, L, **attrs):
    inits = [tensor("W", w)] + ([tensor("B", b)] if b is not None else [])
    return _graph([node("Conv", ["input", "W"] + (["B"] if b is not None else []), ["output"], **attrs)], inits,
                  in_dims=("N", w.shape[1], L))


def test_executor_conv_against_the_reference():
    """Integer data, so the executor's double accumulation is exact and the comparison is equality:
    k in {1, 2, 3, 8}, d in {1, 2, 4, 7}, every auto_pad, asymmetric pads, L in {1, 2, 17}, d (k - 1) >= L."""
    rng = np.random.default_rng(1)
    seen = 0
    for k in (1, 2, 3, 8):
        for d in (1, 2, 4, 7):
            for L in (1, 2, 17):
                span = d * (k - 1)
                x = rng.integers(-3, 4, (2, 3, L)).astype(np.float32)
                w = rng.integers(-2, 3, (5, 3, k)).astype(np.float32)
                b = rng.integers(-4, 5, 5).astype(np.float32)
                cases = [("SAME_UPPER", None, span // 2, span - span // 2), ("SAME_LOWER", None, span - span // 2, span // 2),
                         ("NOTSET", [span, 0], span, 0), ("NOTSET", [1, span + 2], 1, span + 2)]
                if L > span:
                    cases += [("VALID", None, 0, 0), ("NOTSET", None, 0, 0)]
                for ap, pads, pl, pr in cases:
                    attrs = dict(kernel_shape=[k], dilations=[d])
                    if ap != "NOTSET":
                        attrs["auto_pad"] = ap
                    if pads is not None:
                        attrs["pads"] = pads
                    got = _run(_conv_model(w, b if (k + d) % 2 else None, L, **attrs), x)
                    ref = C.ref_conv(x, w, b if (k + d) % 2 else None, d, pl, out_len=L + pl + pr - span)
                    assert got.shape == ref.shape, (k, d, L, ap, pads)
                    np.testing.assert_array_equal(got, ref, err_msg=str((k, d, L, ap, pads)))
                    seen += span >= L
    assert seen > 10


def test_executor_pad_pools_and_reductions():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 4, 9)).astype(np.float32)
    for rank_x, pads in ((x, [0, 1, 2, 1, 0, 3]), (x[0], [2, 0, 0, 5]), (x[0, 0], [3, 1])):
        want = np.pad(rank_x, list(zip(pads[:rank_x.ndim], pads[rank_x.ndim:])), constant_values=1.5)
        dims = ("N",) + rank_x.shape[1:] if rank_x.ndim > 1 else (rank_x.shape[0],)
        m = _graph([node("Pad", ["input", "p", "v"], ["output"])],
                   [tensor("p", np.array(pads, np.int64)), tensor("v", np.array([1.5], np.float32))], in_dims=dims)
        np.testing.assert_array_equal(_run(m, rank_x), want)
        m2 = _graph([node("Pad", ["input"], ["output"], pads=pads, value=1.5, mode="constant")], in_dims=dims)   # opset 2
        np.testing.assert_array_equal(_run(m2, rank_x), want)
    np.testing.assert_array_equal(_run(_graph([node("Pad", ["input", "p"], ["output"])], [tensor("p", np.zeros(6, np.int64))]), x), x)
    x64 = x.astype(np.float64)
    for op, fn in (("GlobalAveragePool", lambda a: a.mean(axis=2, keepdims=True)), ("GlobalMaxPool", lambda a: a.max(axis=2, keepdims=True))):
        np.testing.assert_array_equal(_run(_graph([node(op, ["input"], ["output"])]), x), fn(x64).astype(np.float32))
    for op, fn in (("ReduceMean", np.mean), ("ReduceMax", np.max), ("ReduceSum", np.sum)):
        for axes in ([2], [-1], [1, 2], [0], []):
            for keep in (0, 1):
                want = fn(x64, axis=tuple(axes) if axes else None, keepdims=bool(keep)).astype(np.float32)
                as_attr = _graph([node(op, ["input"], ["output"], keepdims=keep, **({"axes": axes} if axes else {}))])
                as_input = _graph([node(op, ["input", "ax"], ["output"], keepdims=keep)], [tensor("ax", np.array(axes, np.int64))])
                for m in (as_attr, as_input):
                    got = _run(m, x)
                    assert got.shape == np.shape(want), (op, axes, keep)
                    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 if op != "ReduceMax" else 0)
    noop = _graph([node("ReduceSum", ["input", "ax"], ["output"], noop_with_empty_axes=1)], [tensor("ax", np.zeros(0, np.int64))])
    np.testing.assert_array_equal(_run(noop, x), x)
    xn = x.copy()
    xn[1, 2, 0] = xn[2, 3, 8] = np.nan    # the rule of conv.cpp and seq_pool: a NaN in the column makes the maximum NaN
    for m in (_graph([node("GlobalMaxPool", ["input"], ["output"])]), _graph([node("ReduceMax", ["input"], ["output"], axes=[2])])):
        got = _run(m, xn)[:, :, 0]
        assert np.isnan(got[1, 2]) and np.isnan(got[2, 3]) and np.isfinite(np.delete(got.ravel(), [6, 11])).all()


def test_executor_rank3_gather_and_slice():
    x = np.arange(3 * 4 * 9, dtype=np.float32).reshape(3, 4, 9)
    g = lambda idx, axis: _run(_graph([node("Gather", ["input", "i"], ["output"], axis=axis)],
                                      [_scalar("i", idx) if np.ndim(idx) == 0 else tensor("i", np.asarray(idx, np.int64))]), x)
    np.testing.assert_array_equal(g(-1, 2), x[:, :, -1])
    np.testing.assert_array_equal(g(8, -1), x[:, :, 8])
    np.testing.assert_array_equal(g([0, -2, 3], 2), x[:, :, [0, -2, 3]])
    for idx, axis, msg in ((9, 2, "outside"), (0, 1, "only axis 1 / -1 of a 2-D value"), (0, 0, "only axis 1 / -1 of a 2-D value")):
        with pytest.raises(RuntimeError, match=msg):
            g(idx, axis)
    sl = lambda s, e, ax: _run(_graph([node("Slice", ["input", "s", "e", "a"], ["output"])],
                                      [tensor(n_, np.array([v], np.int64)) for n_, v in (("s", s), ("e", e), ("a", ax))]), x)
    np.testing.assert_array_equal(sl(0, -2, 2), x[:, :, :-2])
    np.testing.assert_array_equal(sl(-1, 2 ** 31 - 1, -1), x[:, :, -1:])
    with pytest.raises(RuntimeError, match="only the last axis may be cut"):
        sl(1, 3, 1)


MALFORMED = [
    ("W shape", dict(w=np.zeros((5, 2, 3), np.float32)), "does not match X's 3 channels"),
    ("kernel_shape", dict(kernel_shape=[2]), "differs from W's kernel axis"),
    ("B shape", dict(b=np.zeros(4, np.float32)), "B holds 4 values for 5"),
    ("pads length", dict(pads=[1, 1, 1]), "pads must hold 2 values"),
    ("pads 4", dict(pads=[1, 1, 1, 1]), "pads must hold 2 values"),
    ("negative pads", dict(pads=[-1, 2]), "negative pads"),
    ("dilation 0", dict(dilations=[0]), "a dilation of 0"),
    ("kernel 0", dict(w=np.zeros((5, 3, 0), np.float32), kernel_shape=[0]), "a kernel size of 0"),
    ("group", dict(group=3), "group 3 is not supported"),
    ("stride", dict(strides=[2]), "stride 2 is not supported"),
    ("2-D kernel", dict(w=np.zeros((5, 3, 3, 3), np.float32), kernel_shape=[3, 3]), "only 1-D convolutions"),
    ("auto_pad", dict(auto_pad="SAME"), "unknown auto_pad"),
    ("too long", dict(dilations=[9]), "does not fit"),
]


@pytest.mark.parametrize("what,change,msg", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_conv_is_refused_cleanly(what, change, msg):
    change = dict(change)
    w = change.pop("w", np.ones((5, 3, 3), np.float32))
    b = change.pop("b", np.zeros(5, np.float32))
    attrs = dict(kernel_shape=[3])
    attrs.update(change)
    with pytest.raises(RuntimeError, match=msg):
        _run(_conv_model(w, b, 9, **attrs), np.ones((2, 3, 9), np.float32))


def test_malformed_pad_and_reductions_are_refused_cleanly():
    x = np.ones((2, 3, 9), np.float32)
    for pads, msg in (([0, 0, 1, 0, 0], "5 pads for a value of rank 3"), ([0, 0, -1, 0, 0, 0], "negative pads"),
                      ([0, 0, 2 ** 40, 0, 0, 0], "out of range")):
        with pytest.raises(RuntimeError, match=msg):
            _run(_graph([node("Pad", ["input", "p"], ["output"])], [tensor("p", np.array(pads, np.int64))], in_dims=("N", 3, 9)), x)
    with pytest.raises(RuntimeError, match="constant only"):
        _run(_graph([node("Pad", ["input", "p"], ["output"], mode="reflect")], [tensor("p", np.zeros(6, np.int64))], in_dims=("N", 3, 9)), x)
    with pytest.raises(RuntimeError, match="axis 3 out of range"):
        _run(_graph([node("ReduceMean", ["input"], ["output"], axes=[3])], in_dims=("N", 3, 9)), x)
    with pytest.raises(RuntimeError, match="rank >= 3"):
        _run(_graph([node("GlobalMaxPool", ["input"], ["output"])], in_dims=("N", 3)), x[:, :, 0])


# ------------------------------------------------------------------------------ the builder's spellings
@pytest.mark.parametrize("layout", [0, 1])
def test_three_causal_spellings_agree(layout):
    """pads / chomp / pad_op give bit-identical executor output and identical ConvSteps, and all of it
    is the float64 reference."""
    base = dict(seq=20, in_dim=5, channels=(6, 7), dilations=(1, 3), layout=layout)
    X = C.real_input(layout, n=4, seq=20, in_dim=5)
    outs, plans = [], []
    for style in ("pads", "chomp", "pad_op"):
        m = builders.build("tcn", style=style, **base)
        assert dict((p.key, p.value) for p in m.metadata_props)["family"] == "tcn"
        outs.append(_run(m, X))
        plans.append(compile_onnx(_load(m)))
        assert np.abs(outs[-1] - C.ref_tcn(m, X, **base)).max() <= C.REAL_TOL
        assert np.abs(eval_plan(plans[-1], X) - C.ref_tcn(m, X, **base)).max() < 1e-12
    ops = {style: {n.op_type for n in builders.tcn(style=style, **base).graph.node} for style in ("pads", "chomp", "pad_op")}
    assert "Slice" in ops["chomp"] and "Pad" in ops["pad_op"] and not {"Slice", "Pad"} & ops["pads"]
    for o, p in zip(outs[1:], plans[1:]):
        np.testing.assert_array_equal(o, outs[0])
        assert p.describe() == plans[0].describe()
        for a, b in zip(p.steps, plans[0].steps):
            if a.kind == "conv":
                assert (a.c_in, a.c_out, a.k, a.dil, a.pad_left, a.act, a.res, a.act_post, a.src, a.seq, a.layout) == \
                       (b.c_in, b.c_out, b.k, b.dil, b.pad_left, b.act, b.res, b.act_post, b.src, b.seq, b.layout)
                np.testing.assert_array_equal(a.w_np, b.w_np)
                np.testing.assert_array_equal(a.b_np, b.b_np)


# ------------------------------------------------------------------------------ lowering
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("readout,form,op", [("last", "default", "last"), ("last", "slice", "last"), ("mean", "default", "mean"),
                                             ("mean", "reduce", "mean"), ("max", "default", "max"), ("max", "reduce", "max")])
def test_lowering_steps_and_describe(readout, form, op, layout):
    m = builders.tcn(readout=readout, readout_form=form, layout=layout)
    plan = compile_onnx(_load(m))
    assert plan.describe() == ("conv(16->32,k=3,d=1,p=2) -> conv(32->32,k=3,d=1,p=2) -> conv(16->32,k=1,d=1,p=0) -> "
                               "conv(32->32,k=3,d=2,p=4) -> conv(32->32,k=3,d=2,p=4) -> "
                               f"seqpool({op},32) -> dense(32->1,sigmoid)")
    assert plan.family == "tcn" and plan.seq_input and P.has_sequence(plan.steps) and "conv" in P.SEQUENCE_KINDS
    assert (plan.steps[0].seq, plan.steps[0].layout, plan.steps[0].kind) == (100, layout, "conv")
    assert plan.out_width == 1 and plan.ml_col == 0
    convs = plan.steps[:5]
    assert [(s.act, s.res, s.act_post) for s in convs] == [("relu", None, "none"), ("relu", None, "none"), ("none", 1, "relu"),
                                                           ("relu", None, "none"), ("relu", 2, "relu")]
    assert [P.step_inputs(plan.steps, i) for i in range(7)] == [(-1,), (0,), (-1, 1), (2,), (3, 2), (4,), (5,)]
    assert all(s.out_width == s.c_out and s.w_np.shape == (s.c_out, s.k, s.c_in) for s in convs)
    X = C.real_input(layout)
    assert np.abs(eval_plan(plan, X) - C.ref_tcn(m, X, readout=readout, layout=layout)).max() < 1e-12


def test_lowering_other_shapes_and_folds():
    """No residual, no head, symmetric padding; BatchNormalization folds into the convolution's weights
    (the plan evaluated in float64 equals the reference with the normalisation applied); Sum read-out;
    Dropout / Identity fold away; a second activation takes the post slot."""
    kw = dict(seq=12, in_dim=4, channels=(6, 6), dilations=(1, 2), causal=False, residual=False, head=False, batch_norm=True)
    m = builders.tcn(**kw)
    plan = compile_onnx(_load(m))
    assert plan.describe() == ("conv(4->6,k=3,d=1,p=1) -> conv(6->6,k=3,d=1,p=1) -> conv(6->6,k=3,d=2,p=2) -> "
                               "conv(6->6,k=3,d=2,p=2) -> seqpool(last,6)")
    assert "BatchNormalization" in {n.op_type for n in m.graph.node} and plan.out_width == 6
    X = C.real_input(0, n=3, seq=12, in_dim=4)
    assert np.abs(eval_plan(plan, X) - C.ref_tcn(m, X, **kw)).max() < 1e-6     # folded weights are rounded to f32
    assert np.abs(_run(m, X) - C.ref_tcn(m, X, **kw)).max() < 1e-6
    w = tensor("W", np.ones((3, 4, 2), np.float32))
    nodes = [node("Transpose", ["input"], ["x"], perm=[1, 2, 0]), node("Conv", ["x", "W"], ["c"], kernel_shape=[2], auto_pad="SAME_LOWER"),
             node("Dropout", ["c"], ["dr"]), node("Tanh", ["dr"], ["t"]), node("Identity", ["t"], ["i"]), node("Sigmoid", ["i"], ["s"]),
             node("ReduceSum", ["s", "ax"], ["output"], keepdims=0)]
    g = _graph(nodes, [w, tensor("ax", np.array([2], np.int64))], in_dims=(7, "N", 4), out_rank=2)
    plan = compile_onnx(_load(g))
    assert plan.describe() == "conv(4->3,k=2,d=1,p=1) -> seqpool(sum,3)"
    assert (plan.steps[0].act, plan.steps[0].act_post) == ("tanh", "sigmoid")
    X = C.real_input(0, n=3, seq=7, in_dim=4)
    assert np.abs(eval_plan(plan, X) - _run(g, X)).max() < 1e-6


def test_last_step_slice_directly_behind_a_convolution():
    """Slice[-1:] -> Squeeze with no activation between it and the Conv (or its chomp Slice) is the
    read-out, not part of the layer's padding."""
    W = tensor("W", np.arange(36, dtype=np.float32).reshape(3, 4, 3) / 10)
    i64 = lambda n_, v: tensor(n_, np.array(v, np.int64))
    tail = [node("Slice", ["c", "rs", "re", "a"], ["l3"]), node("Squeeze", ["l3", "a"], ["output"])]
    inits = [W, i64("rs", [-1]), i64("re", [2 ** 31 - 1]), i64("a", [2]), i64("s", [0]), i64("e", [-2])]
    X = C.real_input(0, n=3, seq=9, in_dim=4)
    outs = []
    for body in ([node("Conv", ["x", "W"], ["c"], kernel_shape=[3], pads=[2, 0])],
                 [node("Conv", ["x", "W"], ["f"], kernel_shape=[3], pads=[2, 2]), node("Slice", ["f", "s", "e", "a"], ["c"])]):
        g = _graph([_entry()] + body + tail, inits, in_dims=(9, "N", 4), out_rank=2)
        plan = compile_onnx(_load(g))
        assert plan.describe() == "conv(4->3,k=3,d=1,p=2) -> seqpool(last,3)"
        outs.append(_run(g, X))
        assert np.abs(eval_plan(plan, X) - outs[-1]).max() < 1e-5
    np.testing.assert_array_equal(outs[0], outs[1])


def test_tcn_model_refuses_what_it_cannot_run():
    """runner.TcnModel: only dense layers, in a chain, behind the read-out (the checks come before
    any device allocation)."""
    from dataclasses import replace
    from igaming_platform_amd.engine.runner import TcnModel
    from igaming_platform_amd.models.plan import RowStep
    steps = compile_onnx(_load(builders.tcn(seq=8))).steps
    p = [s.kind for s in steps].index("seqpool")
    for bad, msg in ((steps[:p], "needs a read-out"), (steps[p:], "convolution layers followed by one read-out"),
                     (steps[:p + 1] + [RowStep("softmax", 32)] + steps[p + 1:], "only dense layers behind its read-out, not 'row'"),
                     (steps[:p + 1] + [replace(steps[-1], src=0)], "must form a chain")):
        with pytest.raises(ValueError, match=msg):
            TcnModel(bad, "cpu", True, 8)


def test_native_cpu_abuse_device_only_for_models_it_feeds_right():
    """The C++ CPU abuse device feeds the whole ring in layout 0: a TCN with seq below the ring or a
    batch-major input stays on the Python path (which the engine test below checks)."""
    from igaming_platform_amd.engine.acct import cpu_abuse_native_ok
    ok = lambda m, ring=100: cpu_abuse_native_ok(_load(m), "input", ring)
    assert ok(builders.tcn()) and ok(builders.gru(hidden=8)) and ok(builders.lstm(hidden=8, layout=1))
    assert not ok(builders.tcn(layout=1)) and not ok(builders.tcn(seq=16)) and ok(builders.tcn(seq=16), ring=16)
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.native import native
    for kw, served in ((dict(), True), (dict(layout=1), False)):
        eng = RiskEngine(Config(), backend="cpu", capacity=16, abuse_model=builders.tcn(**kw).SerializeToString())
        if eng.acct is not None:
            assert eng.acct.serves(native().RPC_ABUSE) == served, kw
        eng.close()


def _entry(perm=(1, 2, 0)):
    return node("Transpose", ["input"], ["x"], perm=list(perm))


def _refusal_graphs():
    W = tensor("W", np.ones((4, 4, 3), np.float32))
    W1 = tensor("W1", np.ones((4, 4, 1), np.float32))
    ax2, i64 = tensor("ax2", np.array([2], np.int64)), lambda n_, v: tensor(n_, np.array(v, np.int64))
    conv = lambda x_, y, **a: node("Conv", [x_, "W"], [y], kernel_shape=[3], **a)
    pool = node("GlobalMaxPool", ["c"], ["g"])
    flat = node("Flatten", ["g"], ["output"], axis=1)
    T = (10, "N", 4)
    return [
        ("length", [_entry(), conv("x", "c", pads=[1, 0]), pool, flat], [W], T, "length 9, not T = 10"),
        ("left padding", [_entry(), conv("x", "f", pads=[4, 4]), node("Slice", ["f", "s", "e", "a"], ["c"]), pool, flat],
         [W, i64("s", [6]), i64("e", [16]), i64("a", [2])], T, "left padding of -2"),
        ("pad value", [_entry(), node("Pad", ["x", "p", "v"], ["xp"]), conv("xp", "c"), pool, flat],
         [W, i64("p", [0, 0, 2, 0, 0, 0]), tensor("v", np.array([1.0], np.float32))], T, "non-zero pad value"),
        ("pad on C", [_entry(), node("Pad", ["x", "p"], ["xp"]), conv("xp", "c"), pool, flat],
         [W, i64("p", [0, 1, 2, 0, 0, 0])], T, "padding on N or C"),
        ("strided cut", [_entry(), conv("x", "f", pads=[2, 2]), node("Slice", ["f", "s", "e", "a", "st"], ["c"]), pool, flat],
         [W, i64("s", [0]), i64("e", [12]), i64("a", [2]), i64("st", [2])], T, "not contiguous"),
        ("cut inside", [_entry(), node("Slice", ["x", "s", "e", "a"], ["xs"]), conv("xs", "c", pads=[2, 2]), pool, flat],
         [W, i64("s", [0]), i64("e", [8]), i64("a", [2])], T, "cut inside its T steps"),
        ("other op", [_entry(), conv("x", "c", pads=[2, 0]), node("Softmax", ["c"], ["sm"]), node("GlobalMaxPool", ["sm"], ["g"]), flat],
         [W], T, "op Softmax is not lowered on a sequence value"),
        ("activation shared", [_entry(), conv("x", "c", pads=[2, 0]), node("Relu", ["c"], ["r"]), node("Add", ["c", "r"], ["sum"]),
                               node("GlobalMaxPool", ["sum"], ["g"]), flat], [W], T, "folds only into the convolution producing it"),
        ("add input", [_entry(), conv("x", "c", pads=[2, 0]), node("Add", ["c", "x"], ["sum"]), node("GlobalMaxPool", ["sum"], ["g"]), flat],
         [W], T, "not the model input"),
        ("add constant", [_entry(), conv("x", "c", pads=[2, 0]), node("Add", ["c", "W1"], ["sum"]), node("GlobalMaxPool", ["sum"], ["g"]), flat],
         [W, W1], T, "only the sum of two sequence values"),
        ("two cuts", [_entry(), conv("x", "f", pads=[2, 2]), node("Slice", ["f", "s", "e", "a"], ["c1"]),
                      node("Slice", ["f", "s2", "e2", "a"], ["c2"]), node("Relu", ["c1"], ["r1"]), node("Relu", ["c2"], ["r2"]),
                      node("Add", ["r1", "r2"], ["c"]), pool, flat],
         [W, i64("s", [0]), i64("e", [10]), i64("s2", [2]), i64("e2", [12]), i64("a", [2])], T, "several cuts of one convolution"),
        ("stride", [_entry(), conv("x", "c", pads=[2, 0], strides=[2]), pool, flat], [W], T, "stride 2 is not lowered"),
        ("group", [_entry(), conv("x", "c", pads=[2, 0], group=2), pool, flat], [W], T, "group 2 is not lowered"),
        ("reduce axes", [_entry(), conv("x", "c", pads=[2, 0]), node("ReduceMean", ["c"], ["output"], axes=[1, 2], keepdims=0)], [W], T,
         "time axis \\(axis 2\\) alone"),
        ("gather index", [_entry(), conv("x", "c", pads=[2, 0]), node("Gather", ["c", "i"], ["output"], axis=2)], [W, _scalar("i", 3)], T,
         "only the last step"),
        ("no read-out", [_entry(), node("Conv", ["x", "W"], ["output"], kernel_shape=[3], pads=[2, 0])], [W], T, "a read-out"),
        ("unflattened", [_entry(), conv("x", "c", pads=[2, 0]), pool, node("Gemm", ["g", "Wd"], ["output"])],
         [W, tensor("Wd", np.ones((4, 1), np.float32))], T, "must be flattened"),
        ("row step", [_entry(), conv("x", "c", pads=[2, 0]), pool, node("Flatten", ["g"], ["f"], axis=1), node("Softmax", ["f"], ["output"])],
         [W], T, "row step"),
        ("symbolic T", [_entry(), conv("x", "c", pads=[2, 0]), pool, flat], [W], ("T", "N", 4), "fixed seq"),
        ("T limit", [_entry(), conv("x", "c", pads=[2, 0]), pool, flat], [W], (P.CONV_MAX_T + 1, "N", 4), "time steps"),
    ]


@pytest.mark.parametrize("case", _refusal_graphs(), ids=[c[0] for c in _refusal_graphs()])
def test_lowering_refusals_name_their_reason(case):
    _, nodes, inits, in_dims, msg = case
    with pytest.raises(PlanError, match=msg):
        compile_onnx(_load(_graph(nodes, inits, in_dims=in_dims, out_rank=2)))


def test_limits_and_their_mirror_in_the_kernel_header():
    assert (P.CONV_MAX_C, P.CONV_MAX_K, P.CONV_MAX_SPAN, P.CONV_MAX_T) == (256, 8, 128, 1024)
    src = open(os.path.join(os.path.dirname(__file__), "..", "csrc", "kernels", "launch.h")).read()
    for name in ("CONV_MAX_C", "CONV_MAX_K", "CONV_MAX_SPAN", "CONV_MAX_T"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == getattr(P, name)
    ok = dict(seq=8, in_dim=4, residual=False, head=False)
    assert compile_onnx(_load(builders.tcn(channels=(256,), dilations=(1,), kernel=8, **ok))).steps[0].k == 8
    assert compile_onnx(_load(builders.tcn(channels=(8,), dilations=(64,), kernel=3, **ok))).steps[0].dil == 64
    for kw, msg in ((dict(channels=(257,), dilations=(1,)), "channels"), (dict(channels=(8,), dilations=(1,), kernel=9), "kernel size 9"),
                    (dict(channels=(8,), dilations=(65,), kernel=3), "dilation 65"), (dict(channels=(8,), dilations=(1,), in_dim=257), "channels")):
        m = builders.tcn(**dict(ok, **kw))
        with pytest.raises(PlanError, match=msg):
            compile_onnx(_load(m))
        n = kw.get("in_dim", 4)
        assert _run(m, np.zeros((8, 2, n), np.float32)).shape[0] == 2     # the executor still runs it
    from dataclasses import replace
    s = compile_onnx(_load(builders.tcn(**ok))).steps[0]
    for bad in (replace(s, pad_left=3), replace(s, pad_left=-1), replace(s, res=-1), replace(s, act="gelu"), replace(s, seq=0),
                replace(s, w_np=s.w_np[:1])):
        with pytest.raises(PlanError):
            P.check_conv(bad)
    t = P.conv_tables(s)
    assert tuple(t["w"].shape) == (2, 3, 1, 64, 4) and tuple(t["bias"].shape) == (32,)
    wp = np.zeros((32, 3, 16), np.float32)     # [o, j, c] padded to 16-blocks
    wp[:, :, :4] = s.w_np
    for ob, j, lane, e in ((0, 0, 0, 0), (1, 2, 37, 2), (0, 1, 7, 3), (1, 0, 63, 3), (0, 2, 16, 1)):
        assert t["w"][ob, j, 0, lane, e] == wp[ob * 16 + (lane & 15), j, 4 * (lane >> 4) + e], (ob, j, lane, e)


def test_recurrent_layers_and_conv_do_not_mix():
    inits = [tensor("Wc", np.ones((8, 4, 1), np.float32)), tensor("W1", np.zeros((1, 24, 4), np.float32)),
             tensor("R1", np.zeros((1, 24, 8), np.float32)), tensor("B1", np.zeros((1, 48), np.float32)),
             tensor("shp", np.array([-1, 8], np.int64))]
    nodes = [node("Transpose", ["input"], ["x"], perm=[1, 2, 0]), node("Conv", ["x", "Wc"], ["c"]),
             node("GlobalMaxPool", ["c"], ["gp"]), node("Flatten", ["gp"], ["pooled"], axis=1),
             node("GRU", ["input", "W1", "R1", "B1"], ["Y1", "Yh1"], hidden_size=8), node("Reshape", ["Yh1", "shp"], ["h"])]
    for first, second, op in (("pooled", "h", "GRU"), ("h", "pooled", "Conv")):
        g = _graph(nodes + [node("Add", [first, second], ["output"])], inits, in_dims=(6, "N", 4), out_rank=2)
        assert _run(g, np.zeros((6, 2, 4), np.float32)).shape == (2, 8)
        with pytest.raises(PlanError, match=f"{op}: GRU / LSTM layers and Conv mixed in one model"):
            compile_onnx(_load(g))


# ------------------------------------------------------------------------------ the CPU engine
@pytest.mark.parametrize("layout,seq", [(0, 16), (1, 16), (0, 7)])
def test_cpu_engine_scores_a_tcn_abuse_model(layout, seq):
    """RiskEngine(backend="cpu") with a TCN abuse model: accounts with 0, 1, T - 1, T and more events
    than the ring score what the float64 reference gives on the right-aligned, zero-padded history an
    independent golden store encodes (rounded to the rings' bf16) - also for a batch-major model and
    for one whose graph fixes seq below the 16-entry ring (it reads the last seq steps)."""
    import torch
    from igaming_platform_amd.config import TX_TYPE_ID, Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.golden.features import GoldenFeatureStore, TxEvent
    from igaming_platform_amd.layouts import ACCTBATCH
    cfg = Config()
    cfg.features.event_ring = 16
    kw = dict(seq=seq, layout=layout)
    proto = builders.build("tcn", **kw)
    eng = RiskEngine(cfg, backend="cpu", capacity=50, abuse_model=proto.SerializeToString())
    rows = np.zeros(1, ACCTBATCH)
    rows["present"] = 1
    eng.load_batch_features(["quiet"], rows)
    gold = GoldenFeatureStore(cfg.features)
    evs, counts = [], (("one", 1), ("almost", seq - 1), ("full", seq), ("over", 21))
    for acct, n in counts:
        for i in range(n):
            e = dict(account_id=acct, amount=1000 + 7919 * i, transaction_type=("deposit", "bet", "win")[i % 3], ts=NOW - 400 + 13 * i)
            evs.append(e)
            gold.apply(TxEvent(acct, e["amount"], TX_TYPE_ID[e["transaction_type"]], 0, 0, e["ts"]))
    eng.ingest_events(evs)
    ids = ["quiet"] + [a for a, _ in counts]
    res = eng.check_bonus_abuse_batch(ids, now=NOW)
    X = np.stack([gold.event_history(a) for a in ids], axis=1).astype(np.float32)[-seq:]   # [seq, 5, 16]
    X = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    assert np.count_nonzero(X[:, 0]) == 0 and np.count_nonzero(X[:, 1].any(axis=1)) == 1 and np.all(X[:, 3].any(axis=1))
    ref = C.ref_tcn(proto, X.transpose(1, 0, 2) if layout else X, **kw)[:, 0]
    got = np.array([r.model_score for r in res], np.float64)
    print(f"cpu engine tcn layout {layout} seq {seq}: max err {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= C.REAL_TOL
    assert len(set(np.round(got, 6))) == 5
