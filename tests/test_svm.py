"""ai.onnx.ml SVMClassifier / SVMRegressor on the CPU: the executor against the float64 reference of
tests/svm_cases.py, that reference against scikit-learn itself, the lowering to an ``svm`` plan step
(folds, refusals, host tables) and the CPU engine. Tolerances: the svm_cases docstring."""
import numpy as np
import pytest

from igaming_platform_amd.models.plan import (SVM_MAX_F, PlanError, compile_onnx, executor_output, svm_centre,
                                               svm_tables, validate_svm)
from igaming_platform_amd.native import native
from igaming_platform_amd.onnx import builders
from igaming_platform_amd.onnx import schema as S
from igaming_platform_amd.onnx.writer import ML_DOMAIN, model, node, tensor, value_info
from tests import svm_cases as C


def _run(m, X, name="output"):
    return np.asarray(native().Executor(C.load(m)).run({"input": np.asarray(X, np.float32)})[name])


def _kinds(m):
    return [s.kind for s in compile_onnx(C.load(m)).steps]


# ------------------------------------------------------------------------------ 1: executor against the reference
@pytest.mark.parametrize("post", ["NONE", "LOGISTIC"])
@pytest.mark.parametrize("kernel", C.KERNELS)
def test_executor_regressor_matches_reference(kernel, post):
    for one_class in (False, True):
        m = builders.build("svm", n_features=13, n_sv=37, kernel=kernel, seed=3, one_class=one_class, post=post)
        X = np.random.default_rng(4).standard_normal((41, 13)).astype(np.float32)
        op, a = C.node_attrs(C.load(m))
        ref = C.svm_reference(op, a, X)
        got = _run(m, X)
        assert got.shape == (41, 1) and got.dtype == np.float32
        tol = C.out_tol(op, a, ref, C.dec_tol(ref)) if (one_class or post != "NONE") else C.dec_tol(ref)[:, None]
        assert (np.abs(got - ref["out"]) <= tol).all()
        if one_class:   # the sign itself, off the rows within the rounding of zero
            far = np.abs(ref["dec"]) > C.dec_tol(ref)
            want = C.stage(op, a, ref["dec"])[far, 0]
            assert far.sum() >= 35 and np.allclose(got[far, 0], want, rtol=0, atol=4 * C.ULP)


@pytest.mark.parametrize("platt,post", [(False, "NONE"), (False, "LOGISTIC"), (True, "NONE")])
@pytest.mark.parametrize("kernel", C.KERNELS)
def test_executor_classifier_matches_reference(kernel, platt, post):
    m = builders.build("svm", n_features=13, n_sv=37, kernel=kernel, op="classifier", seed=5, platt=platt, post=post)
    X = np.random.default_rng(6).standard_normal((41, 13)).astype(np.float32)
    op, a = C.node_attrs(C.load(m))
    assert ("prob_a" in a) == platt
    ref = C.svm_reference(op, a, X)
    res = native().Executor(C.load(m)).run({"input": X})
    got, label = np.asarray(res["output"]), np.asarray(res["label"])
    assert got.shape == (41, 2) and label.shape == (41,) and label.dtype == np.int64
    tol = C.dec_tol(ref)[:, None] if (post == "NONE" and not platt) else C.out_tol(op, a, ref, C.dec_tol(ref))
    assert (np.abs(got - ref["out"]) <= tol).all()
    if not platt and post == "NONE":
        np.testing.assert_array_equal(got[:, 1], -got[:, 0])   # [dec, -dec]
    far = np.abs(ref["out"][:, 0] - ref["out"][:, 1]) > 2 * tol.max()
    assert far.sum() >= 35
    np.testing.assert_array_equal(label[far], ref["label"][far])
    assert set(label) <= {0, 1} and (platt or set(label) == {0, 1})


# ------------------------------------------------------------------------------ 2: the reference against scikit-learn
@pytest.mark.parametrize("name", C.SK_CASES)
def test_reference_matches_sklearn(name):
    est, sc, m = C.sk_case(name)
    om = C.load(m)
    op, a = C.node_attrs(om)
    X = C.sk_inputs()
    Xs = C.apply_scaler(C.scaler_attrs(om), X)
    ref = C.svm_reference(op, a, Xs)
    want = C.sk_decision(est, Xs.astype(np.float64))
    tol = C.SKLEARN_TOL * np.abs(np.asarray(a["coefficients"], np.float64)).sum()
    gap = np.abs(ref["dec"] - want).max()
    print(f"{name}: S = {len(a['coefficients'])}, gap {gap:.3g}, bound {tol:.3g}")
    assert gap <= tol and tol < 1e-4 * np.ptp(want)
    if type(est).__name__ == "SVR":
        return
    far = np.abs(want) > tol
    assert far.sum() >= 120
    pred = est.predict(Xs.astype(np.float64))
    if type(est).__name__ == "OneClassSVM":   # predict is the sign of the decision value
        np.testing.assert_array_equal(np.where(ref["dec"] > 0, 1, -1)[far], pred[far])
        return
    if "prob_a" in a:
        # Platt's formula on sklearn's own probA_ / probB_ and float64 decision values
        p0 = 1.0 / (1.0 + np.exp(est.probA_[0] * want + est.probB_[0]))
        lip = abs(est.probA_[0]) / 4 * tol + 1e-6   # |dp/ddec| <= |A| / 4; A and B are rounded to float32
        assert np.abs(ref["out"][:, 0] - p0).max() <= lip
        # predict_proba goes through libsvm's pairwise coupling: a sanity check only
        assert np.abs(ref["out"] - est.predict_proba(Xs.astype(np.float64))).max() <= 5e-3
    else:
        np.testing.assert_array_equal(ref["label"][far], pred[far])
    # the converted model's score column rises with P(classes_[1])
    got = _run(m, X)
    assert got.shape == (len(X), 2) and np.corrcoef(got[:, 1], -want)[0, 1] > 0.9


def test_converter_outputs():
    """OneClassSVM: Sigmoid(-dec), an outlier scores towards 1; SVR: the raw value; "raw" / "label"
    give the bare operator and the +1 / -1 form; a non-binary SVC is refused."""
    from sklearn.svm import SVC
    from igaming_platform_amd.onnx import convert
    X = C.sk_inputs()
    est, sc, m = C.sk_case("ocsvm_rbf")
    Xs = C.apply_scaler(C.scaler_attrs(C.load(m)), X).astype(np.float64)
    dec = est.decision_function(Xs)
    got = _run(m, X)[:, 0]
    np.testing.assert_allclose(got, 1 / (1 + np.exp(dec)), atol=1e-6)
    far_out = X[:5] + 500.0
    assert (_run(m, far_out)[:, 0] > got.mean()).all()
    raw = _run(convert.svm(est, C.N_FEAT, scaler=sc, output="raw"), X)[:, 0]
    np.testing.assert_allclose(raw, dec, atol=1e-5)
    lab = _run(convert.svm(est, C.N_FEAT, scaler=sc, output="label"), X)[:, 0]
    far = np.abs(dec) > 1e-5
    np.testing.assert_array_equal(lab[far], est.predict(Xs)[far])
    est, sc, m = C.sk_case("svr_poly")
    np.testing.assert_allclose(_run(m, X)[:, 0], est.predict(Xs), atol=1e-5)
    d = C.sk_data()
    with pytest.raises(ValueError, match="binary"):
        convert.svm(SVC().fit(d[2][:60], np.arange(60) % 3), C.N_FEAT)


# ------------------------------------------------------------------------------ 3: the plan
@pytest.mark.parametrize("name", C.SK_CASES)
def test_plan_of_converter_outputs(name):
    est, sc, m = C.sk_case(name)
    om = C.load(m)
    plan = compile_onnx(om)
    assert [s.kind for s in plan.steps] == ["svm"] and plan.family == "svm"
    s = plan.steps[0]
    kern = {"rbf": "RBF", "poly": "POLY", "sigmoid": "SIGMOID", "linear": "LINEAR"}[est.kernel]
    assert plan.describe() == f"svm(30,{len(est.support_vectors_)},{kern})"
    # the Scaler is the step's input stage, not a diagonal dense layer
    sa = C.scaler_attrs(om)
    np.testing.assert_allclose(s.in_scale, np.asarray(sa["scale"], np.float64))
    np.testing.assert_allclose(s.in_shift, -np.asarray(sa["offset"], np.float64) * np.asarray(sa["scale"], np.float64))
    clf = type(est).__name__ == "SVC"
    assert (plan.ml_col, plan.executor_col) == ((0, 1) if clf else (0, 0))
    assert executor_output(om) == (1 if clf else 0, "output")
    if name == "svc_platt":
        assert s.platt is not None and s.platt_flip and s.act == "none" and s.post_scale == 1.0
    elif clf:    # the positive column of [sigmoid(dec), sigmoid(-dec)]
        assert s.platt is None and (s.post_scale, s.post_shift, s.act) == (-1.0, 0.0, "sigmoid")
    elif name == "ocsvm_rbf":   # Mul(-1) -> Sigmoid folded into the epilogue
        assert (s.post_scale, s.post_shift, s.act, s.one_class) == (-1.0, 0.0, "sigmoid", False)
    else:
        assert (s.post_scale, s.post_shift, s.act) == (1.0, 0.0, "none")
    # the step, evaluated in float64 from its own fields, is the executor's score column
    X = C.sk_inputs()
    op, a = C.node_attrs(om)
    ref = C.svm_reference(op, a, C.apply_scaler(sa, X))
    want = _run(m, X)[:, plan.executor_col]
    tol = C.step_out_tol(s, ref["dec"], C.dec_tol(ref))
    assert (np.abs(C.step_out(s, ref["dec"]) - want) <= tol).all()
    validate_svm(s)


def _reg(kernel="RBF", tail=(), F=6, S=9, **kw):
    """SVMRegressor -> ``tail`` nodes (each reads the previous value) -> output."""
    rng = np.random.default_rng(1)
    a = dict(kernel_type=kernel, kernel_params=np.array([0.2, 0.5, 2.0], np.float32),
             support_vectors=rng.standard_normal(S * F).astype(np.float32),
             coefficients=rng.standard_normal(S).astype(np.float32),
             rho=np.array([0.1], np.float32), n_supports=S)
    a.update(kw)
    names = ["dec"] + [f"t{i}" for i in range(len(tail))]
    names[-1] = "output"
    nodes = [node("SVMRegressor", ["input"], [names[0]], domain=ML_DOMAIN, **a)]
    inits = []
    for i, t in enumerate(tail):
        if isinstance(t, str):
            nodes.append(node(t, [names[i]], [names[i + 1]]))
        else:
            inits.append(tensor(f"c{i}", np.array([t[1]], np.float32)))
            nodes.append(node(t[0], [names[i], f"c{i}"], [names[i + 1]]))
    return model(nodes, [value_info("input", S_FLOAT, ["N", F])], [value_info("output", S_FLOAT, ["N", 1])], inits,
                 name="svm_test")


S_FLOAT = S.FLOAT


def test_epilogue_folds():
    X = np.random.default_rng(2).standard_normal((20, 6)).astype(np.float32)
    m = _reg(tail=[("Mul", 3.0), ("Add", -0.5), "Neg", "Sigmoid"])
    plan = compile_onnx(C.load(m))
    s = plan.steps[0]
    assert [t.kind for t in plan.steps] == ["svm"] and (s.post_scale, s.post_shift, s.act) == (-3.0, 0.5, "sigmoid")
    op, a = C.node_attrs(C.load(m))
    dec = C.svm_reference(op, a, X)["dec"]
    np.testing.assert_allclose(C.step_out(s, dec), _run(m, X)[:, 0], atol=1e-6)
    # one_class: the sign comes before the folded affine
    m = _reg(tail=[("Mul", -0.25)], one_class=1)
    s = compile_onnx(C.load(m)).steps[0]
    assert s.one_class and s.post_scale == -0.25
    np.testing.assert_allclose(C.step_out(s, C.svm_reference(*C.node_attrs(C.load(m)), X)["dec"]), _run(m, X)[:, 0])
    # post_transform LOGISTIC is the step's activation; what follows it is not folded
    m = _reg(tail=["Sigmoid"], post_transform="LOGISTIC")
    plan = compile_onnx(C.load(m))
    assert [t.kind for t in plan.steps] == ["svm", "row"] and plan.steps[0].act == "sigmoid"


def test_second_reader_forces_a_row_step():
    """dec feeds the Sigmoid and a second branch: the Sigmoid is not folded into the step that
    produces it, and neither is the other branch's Mul."""
    rng = np.random.default_rng(1)
    a = dict(kernel_type="RBF", kernel_params=np.array([0.2, 0.5, 2.0], np.float32),
             support_vectors=rng.standard_normal(54).astype(np.float32), coefficients=rng.standard_normal(9).astype(np.float32),
             rho=np.array([0.1], np.float32), n_supports=9)
    m = model([node("SVMRegressor", ["input"], ["dec"], domain=ML_DOMAIN, **a), node("Sigmoid", ["dec"], ["p"]),
               node("Mul", ["dec", "half"], ["h"]), node("Add", ["p", "h"], ["output"])],
              [value_info("input", S_FLOAT, ["N", 6])], [value_info("output", S_FLOAT, ["N", 1])],
              [tensor("half", np.array([0.5], np.float32))])
    plan = compile_onnx(C.load(m))
    kinds = [t.kind for t in plan.steps]
    s = plan.steps[0]
    assert kinds[:2] == ["svm", "row"] and kinds[-1] == "join" and plan.steps[1].act == "sigmoid"
    assert (s.act, s.post_scale, s.post_shift) == ("none", 1.0, 0.0)
    assert _kinds(_reg(tail=["Sigmoid"])) == ["svm"]


def test_input_affine_folds_through_constant_ops():
    rng = np.random.default_rng(3)
    F, Sn = 6, 9
    a = dict(kernel_type="POLY", kernel_params=np.array([0.2, 0.5, 2.0], np.float32),
             support_vectors=rng.standard_normal(Sn * F).astype(np.float32),
             coefficients=rng.standard_normal(Sn).astype(np.float32), rho=np.array([0.1], np.float32), n_supports=Sn)
    off, sc = rng.standard_normal(F).astype(np.float32), rng.uniform(0.5, 2, F).astype(np.float32)
    m = model([node("Scaler", ["input"], ["x1"], domain=ML_DOMAIN, offset=off, scale=sc),
               node("Mul", ["x1", "two"], ["x2"]), node("SVMRegressor", ["x2"], ["output"], domain=ML_DOMAIN, **a)],
              [value_info("input", S_FLOAT, ["N", F])], [value_info("output", S_FLOAT, ["N", 1])],
              [tensor("two", np.array([2.0], np.float32))])
    plan = compile_onnx(C.load(m))
    s = plan.steps[0]
    assert [t.kind for t in plan.steps] == ["svm"]
    np.testing.assert_allclose(s.in_scale, 2.0 * sc.astype(np.float64))
    np.testing.assert_allclose(s.in_shift, -2.0 * off.astype(np.float64) * sc)
    X = rng.standard_normal((10, F)).astype(np.float32)
    np.testing.assert_allclose(C.expansion_f32(s, X), _run(m, X)[:, 0], rtol=1e-5, atol=1e-5)


def test_plan_refusals():
    """Each is a PlanError; the executor still runs the model."""
    X = np.zeros((2, SVM_MAX_F + 1), np.float32)
    wide = builders.build("svm", n_features=SVM_MAX_F + 1, n_sv=5, kernel="LINEAR")
    with pytest.raises(PlanError, match="CPU-only"):
        compile_onnx(C.load(wide))
    assert _run(wide, X).shape == (2, 1)
    assert _kinds(builders.build("svm", n_features=SVM_MAX_F, n_sv=5, kernel="LINEAR")) == ["svm"]
    for deg in (2.5, 17.0, -1.0):
        m = builders.build("svm", n_features=4, n_sv=5, kernel="POLY", degree=deg)
        with pytest.raises(PlanError, match="degree"):
            compile_onnx(C.load(m))
        assert _run(m, X[:, :4]).shape == (2, 1)
    assert _kinds(builders.build("svm", n_features=4, n_sv=5, kernel="POLY", degree=16.0)) == ["svm"]
    assert _kinds(builders.build("svm", n_features=4, n_sv=5, kernel="RBF", degree=2.5)) == ["svm"]   # unused by RBF
    for post in ("SOFTMAX", "SOFTMAX_ZERO", "PROBIT"):
        for op in ("regressor", "classifier"):
            m = builders.build("svm", n_features=4, n_sv=5, op=op, post=post)
            with pytest.raises(PlanError, match="post_transform"):
                compile_onnx(C.load(m))
    assert _run(builders.build("svm", n_features=4, n_sv=5, op="classifier", post="SOFTMAX"), X[:, :4]).shape == (2, 2)


def _clf(**kw):
    rng = np.random.default_rng(0)
    a = dict(kernel_type="RBF", kernel_params=np.array([0.5, 0.0, 3.0], np.float32),
             support_vectors=rng.standard_normal(12).astype(np.float32), coefficients=rng.standard_normal(4).astype(np.float32),
             rho=np.array([0.1], np.float32), vectors_per_class=np.array([2, 2], np.int64),
             classlabels_ints=np.array([0, 1], np.int64))
    a.update(kw)
    a = {k: v for k, v in a.items() if v is not None}
    return model([node("SVMClassifier", ["input"], ["label", "output"], domain=ML_DOMAIN, **a)],
                 [value_info("input", S_FLOAT, ["N", 3])],
                 [value_info("label", S.INT64, ["N"]), value_info("output", S_FLOAT, ["N", 2])])


MALFORMED = {
    "three classes": (_clf, dict(vectors_per_class=np.array([2, 1, 1], np.int64), classlabels_ints=np.array([0, 1, 2], np.int64),
                                 coefficients=np.ones(8, np.float32), rho=np.ones(3, np.float32)), "more than two classes"),
    "linear SVC form": (_clf, dict(vectors_per_class=None), "linear-SVC"),
    "vectors_per_class sum": (_clf, dict(vectors_per_class=np.array([2, 3], np.int64)), "support_vectors holds"),
    "coefficient count": (_clf, dict(coefficients=np.ones(5, np.float32)), "coefficients for"),
    "kernel_params": (_clf, dict(kernel_params=np.array([0.5, 0.0], np.float32)), "kernel_params"),
    "kernel_type": (_clf, dict(kernel_type="LAPLACE"), "unknown kernel_type"),
    "prob_a alone": (_clf, dict(prob_a=np.array([-1.0], np.float32)), "prob_a and prob_b"),
    "nan vector": (_clf, dict(support_vectors=np.array([np.nan] + [0.0] * 11, np.float32)), "non-finite support vector"),
    "inf coefficient": (_clf, dict(coefficients=np.array([np.inf, 1, 1, 1], np.float32)), "non-finite coefficient"),
    "regressor S*F": (_reg, dict(n_supports=4), "support_vectors holds"),
    "regressor coefficients": (_reg, dict(coefficients=np.ones(3, np.float32)), "coefficients for"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_models_are_refused(case):
    """By the reader (the executor's constructor) and by the plan, with the same message."""
    make, kw, msg = MALFORMED[case]
    om = C.load(make(**kw))
    with pytest.raises(RuntimeError, match=msg):
        native().Executor(om)
    with pytest.raises(PlanError, match=msg):
        compile_onnx(om)


def test_validate_svm_checks_the_step():
    from dataclasses import replace
    s = compile_onnx(C.load(builders.build("svm", n_features=4, n_sv=5, kernel="POLY"))).steps[0]
    validate_svm(s)
    bad = [replace(s, kernel="LAPLACE"), replace(s, degree=17), replace(s, coef_np=s.coef_np[:4]), replace(s, in_dim=5),
           replace(s, sv_np=np.where(np.arange(20).reshape(5, 4) == 3, np.inf, s.sv_np).astype(np.float32)),
           replace(s, in_shift=np.array([0.0, np.nan, 0.0, 0.0])), replace(s, in_scale=np.ones(3)),
           replace(s, gamma=float("nan")), replace(s, act="relu"), replace(s, in_dim=SVM_MAX_F + 1)]
    for b in bad:
        with pytest.raises(PlanError):
            validate_svm(b)


def test_rbf_centring_on_unscaled_features():
    """Features with mean 1e4 and unit spread: the centred float32 expansion stays at the accuracy of
    the scaled problem, where the raw expansion |x|^2 + |s|^2 - 2 x.s (values near 3e9) has lost every
    digit. The table holds s - c, the shift -c, and |s - c|^2 is the table's own."""
    rng = np.random.default_rng(8)
    F, Sn = 30, 100
    sv = (1e4 + rng.standard_normal((Sn, F))).astype(np.float32)
    a = dict(kernel_type="RBF", kernel_params=np.array([1.0 / F, 0.0, 3.0], np.float32), support_vectors=sv.ravel(),
             coefficients=rng.standard_normal(Sn).astype(np.float32), rho=np.array([0.1], np.float32), n_supports=Sn)
    m = model([node("SVMRegressor", ["input"], ["output"], domain=ML_DOMAIN, **a)],
              [value_info("input", S_FLOAT, ["N", F])], [value_info("output", S_FLOAT, ["N", 1])])
    s = compile_onnx(C.load(m)).steps[0]
    c = svm_centre(sv)
    assert np.abs(c - 1e4).max() <= 4 and np.abs(sv.astype(np.float64) - c).max() <= 8
    t = svm_tables(s)
    np.testing.assert_array_equal(t["sv"].numpy()[:Sn, :F], (sv.astype(np.float64) - c).astype(np.float32))
    np.testing.assert_array_equal(t["shift"].numpy()[:F], (-c).astype(np.float32))
    np.testing.assert_array_equal(t["sv_norm"].numpy()[:Sn],
                                  (t["sv"].numpy()[:Sn].astype(np.float64) ** 2).sum(1).astype(np.float32))
    assert not t["sv"].numpy()[Sn:].any() and not t["sv"].numpy()[:, F:].any() and not t["coef"].numpy()[Sn:].any()
    X = (1e4 + rng.standard_normal((64, F))).astype(np.float32)
    ref = C.svm_reference("SVMRegressor", C.node_attrs(C.load(m))[1], X)
    err = np.abs(C.expansion_f32(s, X) - ref["dec"]).max()
    # the scaled problem's bound: |x'|, |s'| <= 8 sqrt(F): d2 carries about F roundings of values up to
    # 3 * 64 F, i.e. F * 2^-24 * 192 F on d2, times gamma = 1 / F, times sum |coef K|
    assert err <= 192 * F * C.EPS * ref["mag"].max()
    assert np.ptp(ref["dec"]) > 0.1
    # a column in which every vector agrees is centred on that value
    sv2 = sv.copy()
    sv2[:, 0] = 12345.0
    assert svm_centre(sv2)[0] == 12345.0
    # integers stay integers (or halves)
    ci = svm_centre(rng.integers(-3, 4, (50, 5)).astype(np.float32))
    assert (ci * 2 == np.round(ci * 2)).all()
    # the other kernels are not centred
    s2 = compile_onnx(C.load(builders.build("svm", n_features=4, n_sv=5, kernel="SIGMOID"))).steps[0]
    t2 = svm_tables(s2)
    np.testing.assert_array_equal(t2["sv"].numpy()[:5, :4], s2.sv_np)
    assert t2["sv_norm"] is None and not t2["shift"].numpy().any() and (t2["scale"].numpy()[:4] == 1).all()


def test_plan_importance_of_an_svm_model():
    from igaming_platform_amd.features.store_ops import plan_importance
    est, sc, m = C.sk_case("svc_linear")
    plan = compile_onnx(C.load(m))
    imp = plan_importance(plan, C.N_FEAT)
    s = plan.steps[0]
    w = np.abs(s.coef_np.astype(np.float64) @ s.sv_np.astype(np.float64))
    assert len(imp) == C.N_FEAT and sum(imp.values()) == pytest.approx(1.0)
    assert list(imp.values())[0] == pytest.approx(w.max() / w.sum())
    # for a linear kernel that is |w| of the primal problem, which sklearn exposes
    np.testing.assert_allclose(w, np.abs(est.coef_[0]), rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------ 4: the CPU engine
def engine_model(name):
    """A kernel machine fitted on the engine's own model inputs (30 features of synthetic traffic)."""
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import SVC, OneClassSVM
    from igaming_platform_amd.onnx import convert
    from tests.test_engine_cpu import _txs
    X = engine_inputs(_txs(300, np.random.default_rng(21))).astype(np.float64)
    sc = StandardScaler().fit(X)
    Xs = ((X.astype(np.float32) - sc.mean_.astype(np.float32)) * (1.0 / sc.scale_).astype(np.float32)).astype(np.float64)
    if name == "ocsvm":
        est = OneClassSVM(kernel="rbf", nu=0.3, gamma="scale").fit(Xs)
    else:
        y = (X[:, np.argmax(X.std(axis=0))] > np.median(X[:, np.argmax(X.std(axis=0))])).astype(int)
        est = SVC(kernel="rbf", probability=True, random_state=0).fit(Xs, y)
    return convert.svm(est, 30, scaler=sc)


def engine_inputs(txs):
    """The fraud model's input rows for a batch scored on an empty feature store."""
    from igaming_platform_amd.config import TX_TYPE_ID, Config
    from igaming_platform_amd.golden.features import GoldenFeatureStore, model_input
    from igaming_platform_amd.utils.hashing import SEED_IP, id_hash
    from tests.test_engine_cpu import NOW
    cfg = Config()
    st = GoldenFeatureStore(cfg.features)
    return np.stack([model_input(st.raw_features(t["account_id"], NOW, ip_hash=id_hash(t["ip_address"], SEED_IP)),
                                 t["amount"], TX_TYPE_ID[t["transaction_type"]], cfg.features.log_transform, 30)
                     for t in txs]).astype(np.float32)


def test_engine_cpu_scores_a_one_class_svm_like_the_executor():
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from tests.test_engine_cpu import NOW, _txs
    m = engine_model("ocsvm")
    eng = RiskEngine(Config(), backend="cpu", capacity=64, fraud_model=m.SerializeToString())
    txs = _txs(60, np.random.default_rng(7))
    got = np.array([r["ml_score"] for r in eng.score(txs, now=NOW)], np.float64)
    assert eng.get_feature_importance()
    eng.close()
    np.testing.assert_allclose(got, _run(m, engine_inputs(txs))[:, 0], rtol=0, atol=1e-6)
    assert np.all((got > 0) & (got < 1)) and np.ptp(got) > 1e-3
