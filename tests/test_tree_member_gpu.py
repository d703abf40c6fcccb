"""BRANCH_MEMBER (mode 6) nodes on the device: K2 (trees.hip: tree_kernel<K, false>, the finish
kernels, tree_head_kernel) and K2b (trees_sparse.hip) against the float64 walk of
tests/tree_member_cases.py, the stacked model in one launch, a scikit-learn
HistGradientBoosting model on both layouts, and an opset-5 fraud model through the engine.

Buffers as in tests/test_tree_edges_gpu.py: X in a NaN-poisoned buffer, the partial slab of every
grouped launch poisoned (NaN; -3e38 / +3e38 for MIN / MAX), outputs pre-filled with a sentinel whose
rows past n_rows must stay bit-identical; 1, 63, 65 and 130 rows. SUM / MIN / MAX cases without a
post transform must EQUAL the reference, the others use rtol = atol = 1e-5. Every case is a few
64-row tiles of small trees."""
from functools import lru_cache

import numpy as np
import pytest

from tests import dense_cases as D
from tests import tree_cases as TC
from tests import tree_member_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _auto_rules(monkeypatch):
    for v in ("IGP_TREE_LAYOUT", "IGP_TREE_GROUPS", "IGP_TREE_HEAD"):
        monkeypatch.delenv(v, raising=False)


def _t():
    import torch
    return torch


def _K():
    from igaming_platform_amd.ops import kernels as K
    return K


def _upload(step, width):
    from igaming_platform_amd.models.plan import Plan, to_device
    to_device(Plan("t", width, [step], step.n_out, 0, {}, "input", "output"), "cuda")
    assert step.sets is not None and step.sets.numel() == step.sets_np.size
    return step


@lru_cache(maxsize=None)
def _case(name):
    b = MC.built(name)
    _upload(b.step, b.case.width)
    return b


@lru_cache(maxsize=None)
def _probe(layout):
    b = MC.built_probe(layout)
    _upload(b.step, MC.PROBE_WIDTH)
    return b


def _poison(aggregate=0):
    return {2: -3e38, 3: 3e38}.get(aggregate, float("nan"))


def _slab(groups, rows, k, aggregate=0):
    torch = _t()
    return torch.full((max(groups, 1) * rows * k,), _poison(aggregate), dtype=torch.float32, device="cuda")


def _launch(step, Xd, Y, rows, g):
    K = _K()
    if step.layout == "sparse":
        K.tree_sparse(step, Xd, Y, rows, partial=_slab(g, rows, step.k, step.aggregate) if g > 1 else None, groups=g)
    else:
        K.tree_ensemble(step, Xd, Y, rows, partial=_slab(g, rows, step.k) if g > 1 else None, groups=g)


def _run_and_compare(step, X, ref, rows, width, groups, exact, what):
    torch = _t()
    Xd = D.poisoned(rows + 9, rows, width, width, torch.float32, np.array(X)).cuda()
    for g in groups:
        Y = D.sentinel_out(rows + 9, step.n_out, torch.float32).cuda()
        _launch(step, Xd, Y, rows, g)
        Y = Y.cpu()
        got = Y[:rows].double().numpy()
        print(f"{what} groups {g} rows {rows}: ratio {TC.ratio(got, ref[:rows]):.4f}")
        if exact:
            np.testing.assert_array_equal(got, ref[:rows], err_msg=f"{what} groups {g}")
        else:
            np.testing.assert_allclose(got, ref[:rows], rtol=TC.RTOL, atol=TC.ATOL, err_msg=f"{what} groups {g}")
        assert D.untouched(Y, rows, Y.shape[1]), f"{what} groups {g}: wrote past n_rows"


# ------------------------------------------------------------------------------ the named sets
@pytest.mark.parametrize("rows", TC.ROWS)
@pytest.mark.parametrize("layout", ["complete", "sparse"])
def test_named_sets_and_their_probes(layout, rows):
    """Every named set (both encodings, word and CAP edges, the empty set, +-0, inf, 1e30) with
    its probes, NaN under both missing tracks, and the set-order tree: K = 64, one group and
    three, exact."""
    b = _probe(layout)
    _run_and_compare(b.step, b.X, b.ref, rows, MC.PROBE_WIDTH, (1, 3), True, f"probe {layout}")


# ------------------------------------------------------------------------------ K2
@pytest.mark.parametrize("rows", TC.ROWS)
@pytest.mark.parametrize("name", [c.name for c in MC.COMPLETE])
def test_complete_layout_member_cases(name, rows):
    """Depth 1 / 3 / 5 / 10, K = 1 / 4 / 32, member nodes at the root, at the last level and among
    all six comparison modes, one group and the grouped launches with a ragged last group, the node
    table in LDS and in global memory (asserted in tests/test_tree_member.py)."""
    b = _case(name)
    _run_and_compare(b.step, b.X, b.ref, rows, b.case.width, b.case.groups, b.case.exact, name)


# ------------------------------------------------------------------------------ K2b
@pytest.mark.parametrize("rows", TC.ROWS)
@pytest.mark.parametrize("name", [c.name for c in MC.SPARSE])
def test_sparse_layout_member_cases(name, rows):
    """A depth-14 chain with member nodes along it beside a single-leaf tree, the X tile staged and
    read from global memory, SUM / AVERAGE / MIN / MAX, one group and three."""
    b = _case(name)
    _run_and_compare(b.step, b.X, b.ref, rows, b.case.width, b.case.groups, b.case.exact, name)


# ------------------------------------------------------------------------------ tree -> head
def test_stacked_member_model_in_one_launch(monkeypatch):
    """Member trees (K = 32) -> f32 head through tree_head_kernel with 3 groups, against the
    two-kernel path (tree_ensemble(no_finish) + mlp_head) and the float64 reference; 130 rows in a
    192-row bucket."""
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    torch, K = _t(), _K()
    trees, head = MC.stacked_member_parts(20)
    om = native().OnnxModel.from_bytes(MC.stacked_member_model(trees, head).SerializeToString())
    plan = to_device(compile_onnx(om), "cuda")
    assert [s.kind for s in plan.steps] == ["tree", "head"] and plan.steps[0].layout == "complete"
    assert not plan.steps[0].all_leq and plan.steps[0].sets is not None
    monkeypatch.setenv("IGP_TREE_GROUPS", "3")
    rows, B = 130, 192    # three tiles, the last one a zero-padded part of the bucket
    X = np.zeros((B, 128), np.float32)
    X[:rows] = MC.make_X(trees, rows, 128, 3)
    ref = MC.stacked_member_ref(trees, head, X[:rows])
    out = {}
    for one in ("1", "0"):
        monkeypatch.setenv("IGP_TREE_HEAD", one)
        dm = DeviceModel(plan, "cuda", [B])
        assert dm.tree_groups[B] == 3 and K.tree_head_ok(plan.steps[0], plan.steps[1], 3)
        dm.tree_partial.fill_(float("nan"))
        y = dm.run(torch.from_numpy(X).cuda(), B)
        torch.cuda.synchronize()
        out[one] = y[:rows, 0].cpu().numpy().copy()
        if one == "1":
            assert int(dm.tile_cnt.abs().sum()) == 0
    np.testing.assert_allclose(out["1"], ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out["0"], ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out["1"], out["0"], atol=1e-5, rtol=0)
    assert np.ptp(ref) > 1e-3


# ------------------------------------------------------------------------------ scikit-learn
@pytest.mark.parametrize("layout", ["complete", "sparse"])
def test_hist_gradient_boosting_classifier_on_the_device(layout, monkeypatch):
    """The scikit-learn model of tests/test_tree_member.py through compile_onnx and the runner on
    both layouts, against the C++ executor."""
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    torch = _t()
    m, raw, _, n_cat, _ = MC.hgb_model("clf")
    assert n_cat > 0
    N = native()
    om = N.OnnxModel.from_bytes(m.SerializeToString())
    monkeypatch.setenv("IGP_TREE_LAYOUT", layout)
    plan = to_device(compile_onnx(om), "cuda")
    assert plan.steps[0].kind == "tree" and plan.steps[0].layout == layout and plan.steps[0].sets is not None
    rows = 256
    X = np.ascontiguousarray(raw[:rows])
    ref = np.asarray(N.Executor(om).run({"input": X})["output"]).reshape(-1)
    dm = DeviceModel(plan, "cuda", [rows])
    out = dm.run(torch.from_numpy(X).cuda(), rows)
    torch.cuda.synchronize()
    got = out[:rows].cpu().numpy().reshape(-1)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)
    assert np.ptp(ref) > 0.1 and np.isnan(X).any()


# ------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("model", ["gbdt_v5", "stacked_v5"])
def test_engine_scores_an_opset5_model_like_the_cpu_backend(model, monkeypatch):
    """Model load path of the engine, gpu against cpu backend: a tree-only opset-5 fraud model (the
    grouped finish with the fused ensemble) and the stacked one (tree_head_kernel -> K5)."""
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    cfg = MC.engine_config()
    if model == "gbdt_v5":
        m = MC.engine_model()
    else:
        trees, head = MC.stacked_member_parts(24)
        m = MC.stacked_member_model(trees, head).SerializeToString()
        cfg.features.width = 128
        monkeypatch.setenv("IGP_TREE_GROUPS", "3")
    g = RiskEngine(cfg, backend="gpu", capacity=1024, fraud_model=m)
    c = RiskEngine(cfg, backend="cpu", capacity=1024, fraud_model=m)
    rng = np.random.default_rng(3)
    for step in range(3):
        txs = MC.engine_txs(200, rng)
        a, b = g.score(txs, now=MC.NOW + 20 * step), c.score(txs, now=MC.NOW + 20 * step)
        np.testing.assert_allclose([x["ml_score"] for x in a], [y["ml_score"] for y in b], atol=1e-5)
        for x, y in zip(a, b):
            assert (x["score"], x["action"], x["reason_codes"], x["rule_score"]) == \
                (y["score"], y["action"], y["reason_codes"], y["rule_score"])
    assert len({y["ml_score"] for y in b}) > 1
    g.close()
    c.close()
