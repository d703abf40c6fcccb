"""Column operators of scikit-learn ColumnTransformer front ends on the CPU: the executor against the
numpy references of tests/column_cases.py (bit-equal), the exporter against scikit-learn's own
``ct.transform``, the lowering to one ``cols`` plan step (views, materialisation rules, refusals, host
check), feature importance through the step and the CPU engine. Bounds: the column_cases docstring."""
import numpy as np
import pytest

from igaming_platform_amd.models.plan import (COL_MAX_IN, COL_MAX_OUT, ColRec, ColumnStep, PlanError, check_columns,
                                               column_table, compile_onnx)
from igaming_platform_amd.onnx import builders
from igaming_platform_amd.onnx import schema as S
from igaming_platform_amd.onnx.writer import ML_DOMAIN, model, node, tensor, value_info
from tests import column_cases as C

NAN = float("nan")


def graph(nodes, n_in, n_out, inits=(), out_type=S.FLOAT, in_type=S.FLOAT, out_shape=None):
    return model(nodes, [value_info("input", in_type, ["N", n_in])],
                 [value_info("output", out_type, out_shape or ["N", n_out])], list(inits), name="columns_test")


def ml(op, ins, outs, **attrs):
    return node(op, ins, outs, domain=ML_DOMAIN, **attrs)


def i64(name, values):
    return tensor(name, np.asarray(values, np.int64))


def scalar(name, value, dtype=np.int64):
    t = tensor(name, np.asarray([value], dtype))
    del t.dims[:]
    return t


def refused(m, X, match):
    with pytest.raises(RuntimeError, match=match):
        C.run(m, X)


X7 = C.probe_matrix(37, 7, seed=1)


# ------------------------------------------------------------------------------ 1: executor against the references
@pytest.mark.parametrize("replaced,values", [(NAN, [0.25]), (NAN, list(np.arange(7) - 3.0)), (C.SENTINEL, [1.5]),
                                             (0.0, [-2.0]), (None, [4.0])])
def test_imputer(replaced, values):
    kw = {} if replaced is None else dict(replaced_value_float=float(replaced))
    m = graph([ml("Imputer", ["input"], ["output"], imputed_value_floats=np.asarray(values, np.float32), **kw)], 7, 7)
    X = X7.copy()
    X[0, :] = [0.0, -0.0, NAN, C.SENTINEL, np.inf, -np.inf, 1.0]
    want = C.ref_imputer(X, values, 0.0 if replaced is None else replaced)
    got = C.run(m, X)
    assert C.same(got, want)
    if replaced == 0.0:
        assert got[0, 0] == -2.0 and got[0, 1] == -2.0      # -0.0 hits 0.0
    if replaced is not None and np.isnan(replaced):
        assert not np.isnan(got).any() and np.isnan(X).any()
    assert C.run(m, np.zeros((0, 7))).shape == (0, 7)


def test_imputer_refusals():
    refused(graph([ml("Imputer", ["input"], ["output"], imputed_value_floats=np.ones(3, np.float32))], 7, 7), X7,
            "Imputer.*1 or C")
    refused(graph([ml("Imputer", ["input"], ["output"])], 7, 7), X7, "Imputer")
    refused(graph([ml("Imputer", ["input"], ["output"], imputed_value_int64s=np.ones(1, np.int64))], 7, 7), X7,
            "Imputer.*int64")
    refused(graph([ml("Imputer", ["input"], ["output"], imputed_value_floats=np.ones(1, np.float32),
                      replaced_value_int64=3)], 7, 7), X7, "Imputer.*int64")


def test_array_feature_extractor():
    idx = [6, 0, 0, 3, 6]
    m = graph([ml("ArrayFeatureExtractor", ["input", "idx"], ["output"])], 7, 5, [i64("idx", [idx])])   # Y [1, 5]: flattened
    assert C.same(C.run(m, X7), X7[:, idx])
    assert C.run(m, np.zeros((0, 7))).shape == (0, 5)
    for bad in ([7], [-1]):
        refused(graph([ml("ArrayFeatureExtractor", ["input", "idx"], ["output"])], 7, 1, [i64("idx", bad)]), X7,
                "ArrayFeatureExtractor.*index")
    refused(graph([ml("ArrayFeatureExtractor", ["input"], ["output"])], 7, 1), X7, "ArrayFeatureExtractor.*missing")
    # indices that are computed, not constants
    nodes = [node("Cast", ["input"], ["ii"], to=S.INT64), ml("ArrayFeatureExtractor", ["input", "ii"], ["output"])]
    refused(graph(nodes, 7, 1), X7, "ArrayFeatureExtractor.*constant")
    refused(graph([ml("ArrayFeatureExtractor", ["input", "idx"], ["output"])], 7, 1,
                  [tensor("idx", np.array([1.0], np.float32))]), X7, "ArrayFeatureExtractor.*integer")


def test_gather():
    for axis in (1, -1):
        for dt in (np.int64, np.int32):
            m = graph([node("Gather", ["input", "idx"], ["output"], axis=axis)], 7, 4,
                      [tensor("idx", np.array([2, -1, -7, 6], dt))])
            assert C.same(C.run(m, X7), X7[:, [2, 6, 0, 6]])
    m = graph([node("Gather", ["input", "idx"], ["output"], axis=1)], 7, 1, [scalar("idx", -2)], out_shape=["N"])
    got = C.run(m, X7)
    assert got.shape == (37,) and C.same(got, X7[:, 5])
    assert C.run(m, np.zeros((0, 7))).shape == (0,)
    refused(graph([node("Gather", ["input", "idx"], ["output"], axis=0)], 7, 7, [i64("idx", [0])]), X7, "Gather.*axis")
    refused(graph([node("Gather", ["input", "idx"], ["output"])], 7, 7, [i64("idx", [0])]), X7, "Gather.*axis")
    for bad in ([7], [-8]):
        refused(graph([node("Gather", ["input", "idx"], ["output"], axis=1)], 7, 1, [i64("idx", bad)]), X7, "Gather.*index")
    nodes = [node("Cast", ["input"], ["ii"], to=S.INT64), node("Gather", ["input", "ii"], ["output"], axis=1)]
    refused(graph(nodes, 7, 1), X7, "Gather.*constant")


@pytest.mark.parametrize("start,end,step", [(0, 3, 1), (2, 100, 2), (-3, 2 ** 63 - 1, 1), (-1, -(2 ** 63), -1), (5, 1, -2),
                                            (6, -8, -3), (3, 3, 1), (-100, 2, 1), (100, -100, -1)])
def test_slice(start, end, step):
    want = X7[:, slice(start, end, step)]
    inits = [i64("s", [start]), i64("e", [end]), i64("a", [-1]), i64("t", [step])]
    m = graph([node("Slice", ["input", "s", "e", "a", "t"], ["output"])], 7, want.shape[1], inits)
    got = C.run(m, X7)
    assert got.shape == want.shape and C.same(got, np.ascontiguousarray(want))


def test_slice_axes_and_refusals():
    # default axes (0, 1) with a full row range; default steps
    m = graph([node("Slice", ["input", "s", "e"], ["output"])], 7, 3, [i64("s", [0, 2]), i64("e", [2 ** 40, 5])])
    assert C.same(C.run(m, X7), np.ascontiguousarray(X7[:, 2:5]))
    m = graph([node("Slice", ["input", "s", "e"], ["output"])], 7, 7, [i64("s", [1, 0]), i64("e", [2 ** 40, 7])])
    refused(m, X7, "Slice.*last axis")
    m = graph([node("Slice", ["input", "s", "e", "a", "t"], ["output"])], 7, 7,
              [i64("s", [0]), i64("e", [7]), i64("a", [1]), i64("t", [0])])
    refused(m, X7, "Slice.*step")
    refused(graph([node("Slice", ["input"], ["output"], starts=[0], ends=[2])], 7, 2), X7, "Slice")
    nodes = [node("Cast", ["input"], ["ii"], to=S.INT64), node("Slice", ["input", "ii", "ii"], ["output"])]
    refused(graph(nodes, 7, 1), X7, "Slice.*constant")
    refused(graph([node("Slice", ["input", "s", "e", "a"], ["output"])], 7, 7,
                  [i64("s", [0]), i64("e", [7]), i64("a", [2])]), X7, "Slice.*axis")


def test_one_hot_encoder_float_probes():
    cats = list(C.CATS)
    m = graph([ml("OneHotEncoder", ["input"], ["output"], cats_int64s=np.asarray(cats, np.int64))], 7, 7,
              out_shape=["N", 7, len(cats)])
    X = X7.copy()
    p = C.probe_values()
    X.ravel()[:len(p)] = p
    got = C.run(m, X)
    assert got.shape == (37, 7, len(cats)) and C.same(got, C.ref_onehot(X, cats))
    one = lambda v: C.run(m, np.full((1, 7), v, np.float32))[0, 0]   # noqa: E731
    assert one(-0.5)[cats.index(0)] == 1 and one(-0.0)[cats.index(0)] == 1       # trunc(-0.5) = -0 matches 0
    assert one(-3.5)[cats.index(-3)] == 1 and one(-1.0)[cats.index(-1)] == 1
    assert one(2.5)[cats.index(2)] == 1 and one(np.nextafter(np.float32(2), np.float32(0)))[cats.index(1)] == 1
    for v in (NAN, np.inf, -np.inf, 2.0 ** 63, -2.0 ** 63, 2.0 ** 24, 2.0 ** 24 + 2):
        assert not one(v).any()
    assert got[..., cats.index(2 ** 24 + 1)].sum() == 0      # no float32 equals 2^24 + 1
    assert C.run(m, np.zeros((0, 7))).shape == (0, 7, len(cats))


def test_one_hot_encoder_int64_rank_and_zeros():
    cats = np.array([4, -2, 2 ** 24 + 1, -2 ** 63], np.int64)
    m = graph([ml("OneHotEncoder", ["input"], ["output"], cats_int64s=cats)], 3, 3, in_type=S.INT64,
              out_shape=["N", 3, 4])
    X = np.array([[4, -2, 0], [2 ** 24 + 1, -2 ** 63, 5]], np.int64)
    assert C.same(C.run(m, X), C.ref_onehot(X, cats))
    assert C.run(m, X)[1, 0, 2] == 1 and C.run(m, X)[1, 1, 3] == 1
    # Cast -> OneHotEncoder: NaN and out-of-range values become INT64_MIN, defined
    nodes = [node("Cast", ["input"], ["i"], to=S.INT64), ml("OneHotEncoder", ["i"], ["output"], cats_int64s=cats[:3])]
    mc = graph(nodes, 7, 7, out_shape=["N", 7, 3])
    Xp = X7.copy()
    Xp.ravel()[:len(C.probe_values())] = C.probe_values()
    assert C.same(C.run(mc, Xp), C.ref_onehot(C.ref_cast_int64(Xp), cats[:3]))
    assert C.same(C.run(mc, Xp), C.ref_onehot(Xp, cats[:3]))     # the same as the float path without INT64_MIN
    cast = graph([node("Cast", ["input"], ["output"], to=S.INT64)], 7, 7, out_type=S.INT64)
    got = C.run(cast, Xp)
    assert got.dtype == np.int64 and np.array_equal(got, C.ref_cast_int64(Xp))
    assert (got[~np.isfinite(Xp)] == np.iinfo(np.int64).min).all()
    # zeros = 0: an unmatched element is a run-time error, a matched batch runs
    mz = graph([ml("OneHotEncoder", ["input"], ["output"], cats_int64s=np.array([0, 1], np.int64), zeros=0)], 2, 2,
               out_shape=["N", 2, 2])
    assert C.same(C.run(mz, [[0, 1], [1.5, 0.25]]), C.ref_onehot(np.array([[0, 1], [1.5, 0.25]], np.float32), [0, 1]))
    refused(mz, [[0, 2]], "OneHotEncoder.*zeros")
    refused(mz, [[NAN, 0]], "OneHotEncoder.*zeros")
    refused(graph([ml("OneHotEncoder", ["input"], ["output"], cats_strings=["a", "b"])], 2, 2), [[0, 1]],
            "OneHotEncoder.*cats_strings")
    refused(graph([ml("OneHotEncoder", ["input"], ["output"])], 2, 2), [[0, 1]], "OneHotEncoder.*cats_int64s")


def test_binarizer():
    X = X7.copy()
    t = np.float32(C.THRESHOLD)
    X[0, :4] = [t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)), NAN]
    m = graph([ml("Binarizer", ["input"], ["output"], threshold=float(t))], 7, 7)
    got = C.run(m, X)
    assert C.same(got, C.ref_binarizer(X, t)) and list(got[0, :4]) == [0, 1, 0, 0]
    m0 = graph([ml("Binarizer", ["input"], ["output"])], 7, 7)
    assert C.same(C.run(m0, X), C.ref_binarizer(X, 0.0))
    assert C.run(m0, np.array([[0.0, -0.0, NAN, 1e-45, -1e-45, np.inf, -np.inf]]))[0].tolist() == [0, 0, 0, 1, 0, 1, 0]


def test_feature_vectorizer():
    nodes = [ml("ArrayFeatureExtractor", ["input", "a"], ["xa"]), node("Gather", ["input", "b"], ["xb"], axis=1),
             node("Cast", ["xa"], ["xi"], to=S.INT64),
             ml("FeatureVectorizer", ["xa", "xb", "input", "xi"], ["output"], inputdimensions=[2, 1, 7, 2])]
    # finite integers, so the int64 input converts exactly
    Xi = np.random.default_rng(5).integers(-9, 10, (37, 7)).astype(np.float32)
    m = graph(nodes, 7, 12, [i64("a", [5, 1]), scalar("b", 3)])
    got = C.run(m, Xi)
    assert C.same(got, np.concatenate([Xi[:, [5, 1]], Xi[:, 3:4], Xi, Xi[:, [5, 1]]], axis=1).astype(np.float32))
    assert C.run(m, np.zeros((0, 7))).shape == (0, 12)
    bad = list(nodes)
    bad[-1] = ml("FeatureVectorizer", ["xa", "xb", "input", "xi"], ["output"], inputdimensions=[2, 2, 7, 2])
    refused(graph(bad, 7, 12, [i64("a", [5, 1]), scalar("b", 3)]), Xi, "FeatureVectorizer.*inputdimensions")
    bad[-1] = ml("FeatureVectorizer", ["xa", "xb"], ["output"], inputdimensions=[2])
    refused(graph(bad, 7, 3, [i64("a", [5, 1]), scalar("b", 3)]), Xi, "FeatureVectorizer.*inputdimensions")


def test_builder_program_matches_the_references():
    """The random program of builders.columns, operator by operator from the references."""
    m = builders.build("columns", final="none", seed=5)
    om = C.load(m)
    nd = {n["outputs"][0]: n for n in om.nodes()}
    X = C.probe_matrix(50, 30, seed=2)
    perm = np.asarray(om.initializer("perm"))
    P = X[:, perm]
    a = lambda name: nd[name]["attrs"]    # noqa: E731
    n_num = len(a("num_i")["imputed_value_floats"])
    num = C.ref_scaler(C.ref_imputer(P[:, :n_num], a("num_i")["imputed_value_floats"], NAN),
                       a("num_s_out")["offset"], a("num_s_out")["scale"])
    c = n_num
    sen = C.ref_imputer(P[:, c:c + 2], a("sen_i")["imputed_value_floats"], C.SENTINEL)
    hot_a = C.ref_onehot(P[:, c + 2], a("hot_a3")["cats_int64s"])
    hot_b = C.ref_onehot(P[:, c + 3], a("hot_b")["cats_int64s"])
    flag = C.ref_binarizer(P[:, c + 4:c + 7], 0.5)
    rest = P[:, :c + 6:-1]
    want = np.concatenate([num, sen, hot_a, hot_b, flag, rest], axis=1)
    got = C.run(m, X)
    assert got.shape[1] == int(om.metadata["assembled_width"]) and C.same(got, want)


# ------------------------------------------------------------------------------ 2: the exporter against scikit-learn
def test_exporter_matches_sklearn_transform():
    ct = C.sk_transformer()
    _, m = C.sk_model("none")
    _, _, Xt = C.sk_data()
    want = np.asarray(ct.transform(Xt), np.float64)
    got = C.run(m, Xt).astype(np.float64)
    assert got.shape == want.shape == (257, C.OUT_WIDTH) == (257, 229)
    assert np.isnan(Xt[:, C.NUM]).mean() > 0.05 and (Xt[:, C.AMT] == C.SENTINEL).mean() > 0.05
    exact = np.arange(C.OUT_WIDTH) >= 13      # one-hot, binarised, passed-through columns
    assert np.array_equal(got[:, exact], want[:, exact])
    assert want[5, 13:21].sum() == 0 and want[6, 21:214].sum() == 0    # the unseen categories
    assert (want[:, 13:13 + sum(C.N_CAT)].sum(axis=1) <= 3).all() and want[:, 13:13 + sum(C.N_CAT)].sum() >= 3 * 255
    bound = C.sk_scaled_bound(want)
    err = np.abs(got - want)
    for name, cols in (("StandardScaler", slice(0, 10)), ("MinMaxScaler", slice(10, 13))):
        ratio = (err[:, cols] / bound[:, cols]).max()
        print(f"{name}: largest |y - y_sk| / bound = {ratio:.3f}")
    assert (err <= bound).all()
    plan = compile_onnx(C.load(m))
    assert plan.describe() == "cols(30->229)" and [s.kind for s in plan.steps] == ["cols"]


def test_exporter_with_a_gradient_boosting_classifier():
    from sklearn.pipeline import make_pipeline
    est, m = C.sk_model("gbc")
    _, _, Xt = C.sk_data()
    pipe = make_pipeline(C.sk_transformer(), est)      # both fitted already
    want = pipe.predict_proba(Xt)[:, 1]
    got = C.run(m, Xt).reshape(-1)
    # rtol = atol = 1e-4: the bound the suite already holds a converted GradientBoostingClassifier to against
    # predict_proba; that test lives in tests/test_native.py (tests/test_onnx_ml.py has no tree estimator)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
    assert np.ptp(want) > 0.5
    plan = compile_onnx(C.load(m))
    assert [s.kind for s in plan.steps] == ["cols", "tree"] and plan.describe().startswith("cols(30->229) -> tree(")


def test_exporter_with_an_rbf_svc():
    from tests import svm_cases as SV
    est, m = C.sk_model("svc")
    _, _, Xt = C.sk_data()
    om = C.load(m)
    Z = C.run(C.sk_model("none")[1], Xt)                  # the assembled matrix, float32, checked above
    op, a = SV.node_attrs(om)
    ref = SV.svm_reference(op, a, Z)
    got = C.run(m, Xt)
    assert got.shape == (257, 2)
    assert (np.abs(got[:, 0] - ref["dec"]) <= SV.dec_tol(ref)).all()            # tests/test_svm.py: executor vs reference
    want = SV.sk_decision(est, Z.astype(np.float64))                          # ... and reference vs scikit-learn
    tol = SV.SKLEARN_TOL * np.abs(np.asarray(a["coefficients"], np.float64)).sum()
    assert np.abs(ref["dec"] - want).max() <= tol and tol < 1e-4 * np.ptp(want)
    # the pipeline's own float64 preprocessing moves the decision value by the scaled columns' rounding only
    from sklearn.pipeline import make_pipeline
    full = -make_pipeline(C.sk_transformer(), est).decision_function(Xt)
    assert np.abs(full - want).max() < 1e-4 * np.ptp(want)
    plan = compile_onnx(om)
    assert [s.kind for s in plan.steps] == ["cols", "svm"]
    _, m2 = C.sk_model("svc_auto")
    p2 = compile_onnx(C.load(m2))
    assert [s.kind for s in p2.steps] == ["cols", "svm"] and (p2.ml_col, p2.executor_col) == (0, 1)


def test_exporter_refusals():
    from sklearn.compose import ColumnTransformer
    from sklearn.preprocessing import OneHotEncoder, PolynomialFeatures, StandardScaler
    from igaming_platform_amd.onnx import convert
    X, y, _ = C.sk_data()
    Xc = np.nan_to_num(X)
    with pytest.raises(ValueError, match="PolynomialFeatures"):
        convert.column_pipeline(ColumnTransformer([("p", PolynomialFeatures(), [0, 1])]).fit(Xc), 30)
    with pytest.raises(ValueError, match="OneHotEncoder"):
        convert.column_pipeline(ColumnTransformer([("c", OneHotEncoder(), [13])]).fit(Xc), 30)     # handle_unknown=error
    with pytest.raises(ValueError, match="OneHotEncoder.*integral"):
        convert.column_pipeline(ColumnTransformer([("c", OneHotEncoder(handle_unknown="ignore"), [16])]).fit(Xc), 30)
    with pytest.raises(ValueError, match="fitted ColumnTransformer"):
        convert.column_pipeline(StandardScaler().fit(Xc), 30)
    ct = ColumnTransformer([("s", StandardScaler(), slice(0, 4))], remainder="passthrough").fit(Xc)
    from sklearn.dummy import DummyClassifier
    with pytest.raises(ValueError, match="DummyClassifier"):
        convert.column_pipeline(ct, 30, final=DummyClassifier().fit(ct.transform(Xc), y))
    m = convert.column_pipeline(ct, 30)
    assert np.abs(C.run(m, Xc) - ct.transform(Xc)).max() < 1e-5
    # a scaler over every column in order and nothing else: Scaler on an identity view
    assert compile_onnx(C.load(m)).describe() == "cols(30->30)"


# ------------------------------------------------------------------------------ 3: lowering
def plan_of(nodes, n_in, n_out, inits=(), **kw):
    return compile_onnx(C.load(graph(nodes, n_in, n_out, inits, **kw)))


def tail(x="asm", k=9):
    """A dense layer reading ``x`` [N, k]: the reader that materialises a view."""
    return [node("Gemm", [x, "W", "B"], ["output"])], [tensor("W", np.ones((k, 1), np.float32)),
                                                        tensor("B", np.zeros(1, np.float32))]


def scaler(x, out, k, off=0.5, sc=2.0):
    return ml("Scaler", [x], [out], offset=np.full(k, off, np.float32), scale=np.full(k, sc, np.float32))


def test_builder_lowers_to_one_cols_step():
    m = builders.build("columns")
    plan = compile_onnx(C.load(m))
    w = int(C.load(m).metadata["assembled_width"])
    assert [s.kind for s in plan.steps] == ["cols", "tree"] and plan.describe().startswith(f"cols(30->{w}) -> tree(")
    s = plan.steps[0]
    assert (s.in_width, s.out_width, len(s.records)) == (30, w, w)
    check_columns(s)
    X = C.probe_matrix(64, 30, seed=3)
    assert C.same(C.eval_records(s.records, X), C.run(builders.build("columns", final="none"), X))
    modes = {r.mode for r in s.records}
    assert modes == {"pass", "onehot", "binarize"} and any(r.imp and r.aff for r in s.records)
    assert any(r.imp and r.imp[0] == C.SENTINEL for r in s.records)
    tab = column_table(s)
    assert tab.dtype.itemsize == 32 and len(tab) == -(-w // 4) * 4 and (tab["src"] < 30).all()


def test_selection_chain_and_identity_view():
    # Gather o Slice o ArrayFeatureExtractor compose into one selection; Concat of views over one base joins records
    inits = [i64("a", [8, 7, 6, 5, 4, 3, 2, 1, 0]), i64("s", [1]), i64("e", [8]), i64("ax", [1]), i64("st", [2]),
             tensor("g", np.array([-1, 0], np.int32))]
    nodes = [ml("ArrayFeatureExtractor", ["input", "a"], ["r"]), node("Slice", ["r", "s", "e", "ax", "st"], ["sl"]),
             node("Gather", ["sl", "g"], ["ga"], axis=1), node("Concat", ["ga", "r", "sl"], ["asm"], axis=1)]
    t, ti = tail(k=15)
    plan = plan_of(nodes + t, 9, 1, inits + ti)
    assert plan.describe() == "cols(9->15) -> dense(15->1,none)"
    assert [r.src for r in plan.steps[0].records] == [1, 7] + [8, 7, 6, 5, 4, 3, 2, 1, 0] + [7, 5, 3, 1]
    assert all(r.identity for r in plan.steps[0].records)
    # the identity over all columns of the base emits nothing; so does a round trip through two reversals
    rev = [node("Slice", ["input", "s", "e", "ax", "st"], ["r1"]), node("Slice", ["r1", "s", "e", "ax", "st"], ["asm"])]
    ri = [i64("s", [-1]), i64("e", [-100]), i64("ax", [-1]), i64("st", [-1])]
    assert plan_of(rev + tail(k=9)[0], 9, 1, ri + tail(k=9)[1]).describe() == "dense(9->1,none)"
    fv = [ml("FeatureVectorizer", ["input"], ["asm"], inputdimensions=[9])]
    assert plan_of(fv + tail(k=9)[0], 9, 1, tail(k=9)[1]).describe() == "dense(9->1,none)"
    # a view as the model output is its step
    assert plan_of([node("Slice", ["input", "s", "e", "ax", "st"], ["output"])], 9, 9, ri).describe() == "cols(9->9)"


def test_one_hot_views():
    cats = np.array([0, 1, 2 ** 24 + 1, 5], np.int64)
    nodes = [ml("ArrayFeatureExtractor", ["input", "a"], ["c"]), ml("OneHotEncoder", ["c"], ["h3"], cats_int64s=cats),
             node("Reshape", ["h3", "shape"], ["h"]), ml("ArrayFeatureExtractor", ["input", "all"], ["x"]),
             node("Concat", ["h", "x"], ["asm"], axis=1)]
    inits = [i64("a", [4, 2]), i64("shape", [0, -1]), i64("all", np.arange(9))]
    plan = plan_of(nodes + tail(k=17)[0], 9, 1, inits + tail(k=17)[1])
    assert plan.describe() == "cols(9->17) -> dense(17->1,none)"
    recs = plan.steps[0].records[:8]      # column-major, then category
    assert [(r.src, r.mode, r.arg) for r in recs] == [(4, "onehot", 0.0), (4, "onehot", 1.0), (4, "zero", 0.0),
                                                      (4, "onehot", 5.0), (2, "onehot", 0.0), (2, "onehot", 1.0),
                                                      (2, "zero", 0.0), (2, "onehot", 5.0)]
    # Cast(int64) as the sole link to the encoder; a scalar Gather gives [N] -> [N, n_cats] directly
    nodes = [node("Gather", ["input", "g"], ["c"], axis=1), node("Cast", ["c"], ["ci"], to=S.INT64),
             ml("OneHotEncoder", ["ci"], ["asm"], cats_int64s=cats)]
    plan = plan_of(nodes + tail(k=4)[0], 9, 1, [scalar("g", 3)] + tail(k=4)[1])
    assert plan.describe() == "cols(9->4) -> dense(4->1,none)" and {r.src for r in plan.steps[0].records} == {3}
    X = C.probe_matrix(40, 9, seed=4)
    assert C.same(C.eval_records(plan.steps[0].records, X), C.ref_onehot(X[:, 3], cats))


def test_materialisation_rules():
    t9, i9 = tail(k=9)
    # Imputer -> Scaler -> Binarizer fills one record
    one = [ml("Imputer", ["input"], ["i"], imputed_value_floats=np.ones(1, np.float32), replaced_value_float=NAN),
           scaler("i", "s", 9), ml("Binarizer", ["s"], ["asm"], threshold=0.25)]
    p = plan_of(one + t9, 9, 1, i9)
    assert p.describe() == "cols(9->9) -> dense(9->1,none)"
    r = p.steps[0].records[4]
    assert r.src == 4 and np.isnan(r.imp[0]) and r.imp[1] == 1.0 and r.aff == (0.5, 2.0) and (r.mode, r.arg) == ("binarize", 0.25)
    # a second affine: the first view is materialised, a fresh one carries the second
    two = [ml("Imputer", ["input"], ["b0"], imputed_value_floats=np.ones(1, np.float32)), scaler("b0", "s1", 9),
           scaler("s1", "s2", 9, 0.25, 3.0), ml("ArrayFeatureExtractor", ["s2", "a"], ["asm"])]
    p = plan_of(two + tail(k=2)[0], 9, 1, [i64("a", [8, 0])] + tail(k=2)[1])
    assert p.describe() == "cols(9->9) -> cols(9->2) -> dense(2->1,none)"
    assert p.steps[0].records[8].aff == (0.5, 2.0) and p.steps[0].records[8].imp == (0.0, 1.0)
    assert [(r.src, r.aff) for r in p.steps[1].records] == [(8, (0.25, 3.0)), (0, (0.25, 3.0))]
    # an Imputer behind a Scaler (the sentinel is compared after the affine, so it cannot move in front of it)
    imp = [ml("ArrayFeatureExtractor", ["input", "all"], ["v"]), scaler("v", "s", 9),
           ml("Imputer", ["s"], ["asm"], imputed_value_floats=np.ones(1, np.float32), replaced_value_float=-3.0)]
    p = plan_of(imp + t9, 9, 1, [i64("all", np.arange(9))] + i9)
    assert p.describe() == "cols(9->9) -> cols(9->9) -> dense(9->1,none)"
    assert p.steps[0].records[2] == ColRec(2, None, (0.5, 2.0)) and p.steps[1].records[2] == ColRec(2, (-3.0, 1.0))
    # a stage already used: Binarizer twice
    bb = [ml("Binarizer", ["input"], ["b1"], threshold=0.5), ml("Binarizer", ["b1"], ["asm"], threshold=0.5)]
    assert plan_of(bb + t9, 9, 1, i9).describe() == "cols(9->9) -> cols(9->9) -> dense(9->1,none)"
    # two operators that each force the same view to materialise share its one step
    t18, i18 = tail(k=18)
    fork = [ml("Binarizer", ["input"], ["b1"], threshold=0.5), ml("Binarizer", ["b1"], ["b2"], threshold=0.25),
            ml("Binarizer", ["b1"], ["b3"], threshold=0.75), node("Concat", ["b2", "b3"], ["asm"], axis=1)]
    assert plan_of(fork + t18, 9, 1, i18).describe() == "cols(9->9) -> cols(9->18) -> dense(18->1,none)"


def test_views_over_two_bases_take_the_join_path():
    inits = [i64("a", [0, 1, 2]), tensor("W0", np.ones((9, 4), np.float32)), tensor("B0", np.zeros(4, np.float32))]
    nodes = [node("Gemm", ["input", "W0", "B0"], ["h"]), node("Relu", ["h"], ["hr"]),
             ml("Binarizer", ["hr"], ["hb"], threshold=0.5), ml("ArrayFeatureExtractor", ["input", "a"], ["sel"]),
             node("Concat", ["hb", "sel"], ["asm"], axis=1)]
    p = plan_of(nodes + tail(k=7)[0], 9, 1, inits + tail(k=7)[1])
    assert [s.kind for s in p.steps] == ["dense", "cols", "cols", "join", "dense"]
    assert p.describe() == "dense(9->4,relu) -> cols(4->4) -> cols(9->3) -> concat(#1,#2) -> dense(7->1,none)"
    # a view beside an ordinary value: the same path
    nodes = [ml("ArrayFeatureExtractor", ["input", "a"], ["sel"]), node("Concat", ["sel", "input"], ["asm"], axis=1)]
    p = plan_of(nodes + tail(k=12)[0], 9, 1, inits[:1] + tail(k=12)[1])
    assert p.describe() == "cols(9->3) -> concat(#0,#-1) -> dense(12->1,none)"
    # a Scaler on a plain value keeps today's lowering (a pending affine folded into the dense layer)
    p = plan_of([scaler("input", "asm", 9)] + tail(k=9)[0], 9, 1, tail(k=9)[1])
    assert p.describe() == "dense(9->1,none)"


def test_plan_refusals():
    t9, i9 = tail(k=9)
    hot = lambda **kw: ml("OneHotEncoder", ["input"], ["h3"], **kw)   # noqa: E731
    cats = dict(cats_int64s=np.array([0, 1, 2], np.int64))
    flat = node("Flatten", ["h3"], ["asm"], axis=1)
    t27, i27 = tail(k=27)

    def no(nodes, inits, match, n_in=9):
        with pytest.raises(PlanError, match=match):
            plan_of(nodes, n_in, 1, inits)
    no([hot(**cats, zeros=0), flat] + t27, i27, "zeros")
    no([hot(cats_strings=["a"]), flat] + t27, i27, "cats_strings")
    no([hot(cats_int64s=np.array([0, -2 ** 63], np.int64)), flat] + tail(k=18)[0], tail(k=18)[1], "INT64_MIN")
    no([hot(**cats), node("Gemm", ["h3", "W", "B"], ["output"])], i27, "flattened")     # 3-D read directly
    no([hot(**cats), ml("Binarizer", ["h3"], ["asm"])] + t27, i27, "flattened")
    no([hot(**cats), node("Squeeze", ["h3"], ["asm"])] + t27, i27, "flattened")
    no([ml("Imputer", ["input"], ["asm"], imputed_value_int64s=np.ones(1, np.int64))] + t9, i9, "int64")
    no([ml("Imputer", ["input"], ["asm"], imputed_value_floats=np.ones(2, np.float32))] + t9, i9, "imputed_value_floats")
    no([ml("ArrayFeatureExtractor", ["input", "a"], ["asm"])] + t9, [i64("a", [9])] + i9, "index")
    no([ml("ArrayFeatureExtractor", ["input", "a"], ["asm"])] + t9, [tensor("a", np.zeros(1, np.int32))] + i9, "int64")
    no([node("Gather", ["input", "a"], ["asm"], axis=0)] + t9, [i64("a", [0])] + i9, "axis")
    no([node("Gather", ["input", "a"], ["asm"], axis=1)] + t9, [i64("a", [-10])] + i9, "index")
    no([node("Relu", ["input"], ["ii"]), node("Gather", ["input", "ii"], ["asm"], axis=1)] + t9, i9, "constant")
    no([node("Gather", ["input", "a"], ["asm"], axis=1)] + tail(k=1)[0], [scalar("a", 2)] + tail(k=1)[1], "scalar index")
    no([node("Slice", ["input", "s", "e", "ax"], ["asm"])] + t9, [i64("s", [1]), i64("e", [2 ** 40]), i64("ax", [0])] + i9,
       "last axis")
    no([node("Slice", ["input", "s", "e", "ax", "st"], ["asm"])] + t9,
       [i64("s", [0]), i64("e", [9]), i64("ax", [1]), i64("st", [0])] + i9, "step")
    no([node("Slice", ["input", "s", "e", "ax"], ["asm"])] + t9, [i64("s", [0, 1]), i64("e", [9, 5]), i64("ax", [1, -1])] + i9,
       "named twice")
    no([ml("FeatureVectorizer", ["input"], ["asm"], inputdimensions=[8])] + t9, i9, "inputdimensions")
    no([node("Cast", ["input"], ["asm"], to=S.INT64)] + t9, i9, "Cast to a non-float")
    # limits: unknown width, in_width > 256, out_width > 4096
    m = model([ml("Binarizer", ["input"], ["asm"])] + t9, [value_info("input", S.FLOAT, ["N", "F"])],
              [value_info("output", S.FLOAT, ["N", 1])], i9)
    with pytest.raises(PlanError, match="unknown width"):
        compile_onnx(C.load(m))
    w = COL_MAX_IN + 1
    no([ml("Binarizer", ["input"], ["asm"])] + tail(k=w)[0], tail(k=w)[1], "CPU-only", n_in=w)
    big = np.arange(COL_MAX_OUT // 9 + 1, dtype=np.int64)
    k = 9 * len(big)
    no([hot(cats_int64s=big), flat] + tail(k=k)[0], tail(k=k)[1], "4096")
    assert COL_MAX_IN == 256 and COL_MAX_OUT == 4096


def test_check_columns_on_corrupted_tables():
    good = ColumnStep(4, 3, [ColRec(0), ColRec(3, (NAN, 1.0), (0.5, 2.0), "onehot", 2.0), ColRec(1, None, None, "binarize", 0.5)])
    check_columns(good)
    tab = column_table(good)
    assert len(tab) == 4 and tab["flags"].tolist() == [0, 0x10 | 0x20 | 0x40 | 1, 2, 3] and tab["src"].tolist() == [0, 3, 1, 0]

    def bad(match, **kw):
        recs = kw.pop("records", good.records)
        with pytest.raises(PlanError, match=match):
            check_columns(ColumnStep(kw.pop("in_width", 4), kw.pop("out_width", len(recs)), recs))
    bad("source column", records=[ColRec(4)])
    bad("source column", records=[ColRec(-1)])
    bad("unknown mode", records=[ColRec(0, None, None, "square")])
    bad("non-finite affine", records=[ColRec(0, None, (0.0, float("inf")))])
    bad("non-finite affine", records=[ColRec(0, None, (NAN, 1.0))])
    bad("non-finite constant", records=[ColRec(0, None, None, "binarize", NAN)])
    bad("one-hot category", records=[ColRec(0, None, None, "onehot", 0.5)])
    bad("one-hot category", records=[ColRec(0, None, None, "onehot", -2.0 ** 63)])
    bad("output columns", out_width=2)
    bad("input columns", in_width=257)
    bad("input columns", in_width=0, records=[ColRec(0)])
    bad("output columns", records=[ColRec(0)] * 4097)


# Every builders family that existed before the column operators, as the lowering rules of the commit
# before them compiled it (recorded by compiling each family with that commit's models/plan.py):
# describe(), family, ml_col, executor_col, out_width and a CRC-32 over every host array of every step
# (field name + bytes, in step and field order), so weights, biases and tables are compared too.
FAMILIES = {
    "qdq_mlp": ("quant(30,uint8) -> qdense(uint8:30->64,relu,uint8) -> qdense(uint8:64->1,sigmoid,f32)",
        "mlp", 0, 0, 1, 0x8780f19a),
    "logistic": ("dense(32->1,sigmoid)",
        "logistic", 0, 0, 1, 0xf376d7af),
    "gbdt": ("tree(T=100,D=7,K=1,post=1,complete)",
        "gbdt", 1, 1, 2, 0x30598510),
    "gbdt_v5": ("tree(T=50,D=5,K=1,post=1,complete)",
        "gbdt", 0, 0, 1, 0xdc7b8f8a),
    "stacked": ("tree(T=100,D=7,K=32,post=0,complete) -> head(32->256,relu->1,sigmoid)",
        "stacked", 0, 0, 1, 0x8fa7524b),
    "ltv_mlp": ("dense(256->512,relu) -> dense(512->512,relu) -> dense(512->512,relu) -> head(512->512,relu->1,none)",
        "mlp", 0, 0, 1, 0x4539dc94),
    "gru": ("gru(I=16,H=256) -> gru(I=256,H=256) -> dense(256->1,sigmoid)",
        "gru", 0, 0, 1, 0x5531bade),
    "lstm": ("lstm(I=16,H=256) -> lstm(I=256,H=256) -> dense(256->1,sigmoid)",
        "lstm", 0, 0, 1, 0xd0ad5083),
    "torch_mlp": ("dense(32->64,relu) -> head(64->64,relu->1,sigmoid)",
        "mlp", 0, 1, 1, 0x15725d4b),
    "tabular_resnet": ("dense(32->128,none) -> layernorm(128) -> dense(128->128,relu) -> dense(128->128,none) -> add(#0,#3) -> relu(128) -> layernorm(128) -> dense(128->128,relu) -> dense(128->128,none) -> add(#5,#8) -> relu(128) -> layernorm(128) -> relu(128) -> dense(128->1,sigmoid)",
        "mlp", 0, 0, 1, 0xa79cfd51),
    "sklearn_linear": ("dense(32->1,sigmoid)",
        "linear", 0, 1, 1, 0x18773a88),
    "linear_regressor": ("dense(32->1,none)",
        "linear", 0, 0, 1, 0xd89e8677),
    "mlp_classifier": ("head(32->64,relu->1,sigmoid)",
        "mlp", 0, 1, 1, 0x85ce4669),
    "wide_deep": ("dense(32->128,relu) -> dense(128->64,relu) -> dense(32->16,none) -> concat(#1,#2) -> dense(80->1,sigmoid)",
        "mlp", 0, 0, 1, 0xa917ea3f),
    "residual_mlp": ("dense(32->128,relu) -> dense(128->128,relu) -> dense(128->128,relu) -> add(#0,#2) -> dense(128->128,relu) -> dense(128->128,relu) -> add(#3,#5) -> dense(128->1,sigmoid)",
        "mlp", 0, 0, 1, 0x044618e2),
    "svm": ("svm(30,100,RBF)",
        "svm", 0, 0, 1, 0x75a72221),
}


def plan_fingerprint(plan):
    import dataclasses
    import zlib
    crc = 0
    for s in plan.steps:
        for f in dataclasses.fields(s):
            v = getattr(s, f.name)
            if isinstance(v, np.ndarray):
                crc = zlib.crc32(np.ascontiguousarray(v).tobytes(), zlib.crc32(f.name.encode(), crc))
    return crc


def test_graphs_without_column_operators_lower_as_before():
    """Every earlier family compiles to the plan recorded in FAMILIES, step for step: such graphs do
    pass through changed code (the Concat / FeatureVectorizer pre-branch, the Cast branch of the alias
    ops, the family detection, the final get() on the output), and none of it may change them."""
    assert set(FAMILIES) == set(builders.BUILDERS) - {"columns"}
    for kind, (describe, family, ml_col, executor_col, out_width, crc) in FAMILIES.items():
        om = C.load(builders.build(kind))
        ops = {n["op_type"] for n in om.nodes()}
        assert not ops & {"Imputer", "ArrayFeatureExtractor", "Gather", "Slice", "OneHotEncoder", "Binarizer",
                          "FeatureVectorizer"}
        plan = compile_onnx(om)
        assert all(s.kind != "cols" for s in plan.steps), kind
        assert plan.describe() == describe, kind
        assert (plan.family, plan.ml_col, plan.executor_col, plan.out_width) == (family, ml_col, executor_col, out_width), kind
        assert plan_fingerprint(plan) == crc, kind


def test_plan_importance_through_a_cols_step():
    from igaming_platform_amd.features.store_ops import input_names, plan_importance
    # trees: a split on assembled column j counts for the input column its record reads
    plan = compile_onnx(C.load(builders.build("columns", seed=9)))
    cols, tree = plan.steps
    nodes = np.asarray(tree.nodes_np, np.float32).reshape(-1, 2)
    feat = (nodes[:, 1].view(np.uint32)[np.isfinite(nodes[:, 0])] & 0xFFFF).astype(np.int64)
    want = np.bincount(np.array([r.src for r in cols.records])[feat], minlength=30).astype(np.float64)
    imp = plan_importance(plan, 30)
    names = input_names(30)
    assert sum(imp.values()) == pytest.approx(1.0)
    for j in range(30):
        assert imp.get(names[j], 0.0) == pytest.approx(want[j] / want.sum())
    assert cols.out_width > 30 and feat.max() >= 30      # bincount(...)[:30] alone would have dropped these
    # a first dense layer: column L1 norms through the records (two assembled columns read input column 2)
    w = np.arange(1.0, 5.0, dtype=np.float32)[:, None]
    nodes_ = [ml("ArrayFeatureExtractor", ["input", "a"], ["asm"]), node("Gemm", ["asm", "W", "B"], ["output"])]
    p = plan_of(nodes_, 6, 1, [i64("a", [2, 5, 2, 0]), tensor("W", w), tensor("B", np.zeros(1, np.float32))])
    imp = plan_importance(p, 6)
    n6 = input_names(6)
    assert imp == pytest.approx({n6[2]: 0.4, n6[5]: 0.2, n6[0]: 0.4})
    # a kernel machine behind the step (the exported SVC pipeline): |sum_i coef_i sv_i| through the records
    plan = compile_onnx(C.load(C.sk_model("svc")[1]))
    cols, sv = plan.steps
    w = np.abs(sv.coef_np.astype(np.float64) @ sv.sv_np.astype(np.float64))
    want = np.bincount(np.array([r.src for r in cols.records]), weights=w, minlength=30)
    imp = plan_importance(plan, 30)
    assert sum(imp.values()) == pytest.approx(1.0) and want[26:].sum() == 0 and len(imp) == 26    # 26 .. 29 are dropped
    for j in range(30):
        assert imp.get(names[j], 0.0) == pytest.approx(want[j] / want.sum())


# ------------------------------------------------------------------------------ 4: the CPU engine
def engine_model():
    """A ColumnTransformer + gradient boosting pipeline fitted on the engine's own model inputs."""
    from sklearn.compose import ColumnTransformer
    from sklearn.ensemble import GradientBoostingClassifier
    from sklearn.preprocessing import Binarizer, OneHotEncoder, StandardScaler
    from igaming_platform_amd.onnx import convert
    from tests.test_engine_cpu import _txs
    from tests.test_svm import engine_inputs
    X = engine_inputs(_txs(300, np.random.default_rng(21))).astype(np.float64)
    ct = ColumnTransformer([("amount", StandardScaler(), [26, 3, 10]),
                            ("type", OneHotEncoder(handle_unknown="ignore"), [27, 28]),
                            ("bet", Binarizer(threshold=0.5), [29])], remainder="passthrough").fit(X)
    y = (X[:, 26] > np.median(X[:, 26])).astype(int)
    est = GradientBoostingClassifier(n_estimators=20, max_depth=3, random_state=0).fit(ct.transform(X), y)
    return convert.column_pipeline(ct, 30, final=est)


def test_engine_cpu_scores_through_the_pipeline_model():
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from tests.test_engine_cpu import NOW, _txs
    from tests.test_svm import engine_inputs
    m = engine_model()
    assert compile_onnx(C.load(m)).describe().startswith("cols(30->32) -> tree(")
    eng = RiskEngine(Config(), backend="cpu", capacity=64, fraud_model=m.SerializeToString())
    txs = _txs(60, np.random.default_rng(7))
    got = np.array([r["ml_score"] for r in eng.score(txs, now=NOW)], np.float64)
    assert eng.get_feature_importance()
    eng.close()
    np.testing.assert_allclose(got, C.run(m, engine_inputs(txs))[:, 0], rtol=0, atol=1e-6)
    assert np.all((got > 0) & (got < 1)) and np.ptp(got) > 1e-3
