"""The K3 edge cases of tests/dense_cases.py on the C++ CPU executor against the float64
reference: pins the executor (the device's failover twin) at the same odd shapes, and checks the
reference helper and the case tables without a GPU."""
import numpy as np
import pytest

from tests import dense_cases as D

TOL = dict(rtol=1e-5, atol=1e-5)


def _run(model_bytes, X):
    from igaming_platform_amd.native import native
    N = native()
    om = N.OnnxModel.from_bytes(model_bytes)
    return np.asarray(N.Executor(om).run({"input": np.ascontiguousarray(X, np.float32)})["output"])


@pytest.mark.parametrize("case", D.DENSE_CASES + [D.DENSE_YBF16], ids=D.dense_id)
def test_executor_dense_matches_float64(case):
    X, W, b = D.dense_operands(case)
    got = _run(D.onnx_mlp([(W, b, case[3])]), X)
    np.testing.assert_allclose(got, D.ref64(X, [(W, b, case[3])]), **TOL)


@pytest.mark.parametrize("case", D.HEAD_CASES, ids=D.head_id)
def test_executor_head_matches_float64(case):
    _, K, N1, act1, act2, xbf = case[:6]
    X, W1, b1, w2, b2 = D.head_operands(K, N1, xbf=xbf)
    head = (W1, b1, act1, w2, b2, act2)
    got = _run(D.onnx_mlp(D.head_layers(head)), X)
    np.testing.assert_allclose(got, D.ref64(X, head=head), **TOL)


@pytest.mark.parametrize("name", list(D.CHAIN_CASES))
def test_executor_chain_matches_float64(name):
    X, lay, head = D.chain_operands(name)
    got = _run(D.onnx_mlp(lay + D.head_layers(head)), X)
    np.testing.assert_allclose(got, D.ref64(X, lay, head), **TOL)


@pytest.mark.parametrize("kind,kw,kinds", D.MODEL_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(D.MODEL_CASES)])
def test_executor_odd_models_match_float64_of_their_plan(kind, kw, kinds):
    """The lowered plan (Scaler folded, head fused) in float64 equals the executor on the ONNX graph."""
    from igaming_platform_amd.models.plan import compile_onnx
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    N = native()
    om = N.OnnxModel.from_bytes(builders.build(kind, **kw).SerializeToString())
    plan = compile_onnx(om)
    assert [s.kind for s in plan.steps] == kinds
    X = np.random.default_rng(11).standard_normal((64, kw["n_features"])).astype(np.float32)
    got = np.asarray(N.Executor(om).run({"input": X})["output"]).reshape(64, -1)[:, plan.executor_col]
    lay, head = D.plan_layers(plan)
    np.testing.assert_allclose(got, D.ref64(X, lay, head)[:, plan.ml_col], **TOL)


def test_reference_conventions():
    """bf16r is round-to-nearest-even; the bf16 convention rounds between layers, not the head's
    hidden layer; relu of NaN is 0 (x > 0 ? x : 0, as the executor and the kernels compute it)."""
    assert D.bf16r(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])).tolist() == [1.0, 1.0 + 2.0 ** -6]
    assert D.act64("relu", np.array([np.nan, -1.0, 2.0])).tolist() == [0.0, 0.0, 2.0]
    X, lay, head = D.chain_operands("30-64-64")
    h = D.bf16r(D.act64(lay[0][2], D.bf16r(X) @ D.bf16r(lay[0][0]).T + lay[0][1]))
    z = D.act64(head[2], h @ D.bf16r(head[0]).T + head[1])
    want = D.act64(head[5], z @ head[3].astype(np.float64) + head[4])
    np.testing.assert_array_equal(D.ref64(X, lay, head, bf16=True)[:, 0], want)
    Xs = D.saturating_rows(X, lay[0][0], lay[0][1], range(8, 16))
    z = Xs[8:16].astype(np.float64) @ lay[0][0].astype(np.float64).T + lay[0][1]
    assert np.abs(z).min() >= 50 and np.abs(z).max() > 1e4
    np.testing.assert_array_equal(Xs[:8], X[:8])
