"""scikit-learn tree ensembles, kernel machines and ColumnTransformer front ends -> ONNX
``ai.onnx.ml`` models.

Stands in for the reference's missing model export scripts (Makefile:215-225
``model-train``/``model-export``; the scripts are not in the repository) and is the
independent oracle for the tree kernels: a model fitted by sklearn,
exported here, must score identically in the C++ executor and on the GPU.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import schema as S
from .writer import V5_AGGREGATE, V5_POST, model, node, tensor, tree_attrs, tree_attrs_v5, value_info


def _tree_dict(tree, scale: float, k_index: int = 0, n_targets: int = 1):
    t = tree.tree_
    n = t.node_count
    feat = np.where(t.children_left < 0, -1, t.feature).astype(np.int64)
    vals = np.zeros((n, n_targets), np.float32)
    vals[:, k_index] = t.value[:, 0, 0] * scale if t.value.ndim == 3 else t.value[:, 0] * scale
    return dict(feature=feat, threshold=t.threshold.astype(np.float32), left=t.children_left, right=t.children_right,
                mode=["BRANCH_LEQ"] * n, missing_true=np.zeros(n, np.int64), leaf_values=vals)


def gradient_boosting(est, n_features: int, input_name: str = "input", output_name: str = "output"):
    """GradientBoostingRegressor / binary GradientBoostingClassifier -> ONNX.

    Regressor: TreeEnsembleRegressor (n_targets=1, base = init prediction).
    Binary classifier: TreeEnsembleRegressor on the log-odds + Sigmoid -> P(class 1) [N, 1].
    sklearn sends ``x <= threshold`` left, which is ONNX BRANCH_LEQ with the true branch left.
    """
    lr = float(est.learning_rate)
    trees: List[dict] = [_tree_dict(t[0], lr) for t in est.estimators_]
    X0 = np.zeros((1, n_features), np.float32)
    base = float(np.asarray(est._raw_predict_init(X0)).ravel()[0])
    a = tree_attrs(trees, "target")
    a.update(n_targets=1, aggregate_function="SUM", post_transform="NONE", base_values=np.array([base], np.float32))
    is_clf = hasattr(est, "classes_")
    if is_clf and len(est.classes_) != 2:
        raise ValueError("only binary classifiers are converted")
    nodes = [node("TreeEnsembleRegressor", [input_name], ["raw" if is_clf else output_name], domain="ai.onnx.ml", **a)]
    if is_clf:
        nodes.append(node("Sigmoid", ["raw"], [output_name]))
    return model(nodes, [value_info(input_name, S.FLOAT, ["N", n_features])],
                 [value_info(output_name, S.FLOAT, ["N", 1])], name="sklearn_gbdt",
                 metadata={"family": "gbdt", "source": "sklearn"})


def random_forest(est, n_features: int, input_name: str = "input", output_name: str = "output",
                  aggregate: str = "AVERAGE", post_transform: str = "NONE"):
    """RandomForestRegressor -> TreeEnsembleRegressor with AVERAGE aggregation (``aggregate``
    MIN / MAX / SUM and a ``post_transform`` give the other TreeEnsemble variants over the same
    fitted trees: the device parity tests use them)."""
    trees = [_tree_dict(t, 1.0) for t in est.estimators_]
    a = tree_attrs(trees, "target")
    a.update(n_targets=1, aggregate_function=aggregate, post_transform=post_transform)
    return model([node("TreeEnsembleRegressor", [input_name], [output_name], domain="ai.onnx.ml", **a)],
                 [value_info(input_name, S.FLOAT, ["N", n_features])],
                 [value_info(output_name, S.FLOAT, ["N", 1])], name="sklearn_rf", metadata={"family": "gbdt"})


def hist_gradient_boosting(est, n_features: int, input_name: str = "input", output_name: str = "output",
                           categories: Optional[Dict[int, Sequence[float]]] = None):
    """HistGradientBoostingRegressor / binary HistGradientBoostingClassifier -> ONNX with the
    opset-5 ``TreeEnsemble`` operator (+ Sigmoid for the classifier: P(class 1) [N, 1]).

    A numeric node is BRANCH_LEQ on ``num_threshold`` (true branch = left); a categorical node is
    BRANCH_MEMBER on the categories set in its row of ``raw_left_cat_bitsets``;
    ``missing_go_to_left`` becomes ``missing_value_tracks_true``. The operator has no base values:
    the baseline prediction is added to the leaves of the first tree. Thresholds and leaf values
    are rounded to float32.

    One difference: scikit-learn sends a non-NaN category that was not among the training
    categories the way missing values go; the operator tests membership only, so such a value
    takes the false branch. Inputs within the training categories (and NaN) score as in sklearn.

    ``categories``: feature index -> the raw input value of each ordinal code the estimator was
    fitted on (an OrdinalEncoder in front of the estimator, folded into the member sets): the
    exported model then reads the raw values."""
    is_clf = hasattr(est, "classes_")
    if is_clf and len(est.classes_) != 2:
        raise ValueError("only binary classifiers are converted")
    base = float(np.asarray(est._baseline_prediction).ravel()[0])
    trees: List[dict] = []
    for it, preds in enumerate(est._predictors):
        p = preds[0]
        nd, bitsets = p.nodes, p.raw_left_cat_bitsets
        n = len(nd)
        leaf = nd["is_leaf"].astype(bool)
        cat = nd["is_categorical"].astype(bool) & ~leaf
        vals = np.zeros((n, 1), np.float64)
        vals[leaf, 0] = nd["value"][leaf] + (base if it == 0 else 0.0)
        members = [None] * n
        for i in np.flatnonzero(cat):
            words = bitsets[int(nd["bitset_idx"][i])]
            codes = [32 * w + b for w in range(len(words)) for b in range(32) if (int(words[w]) >> b) & 1]
            raw = (categories or {}).get(int(nd["feature_idx"][i]))
            if raw is not None:  # codes past the encoder's categories cannot occur in its output
                codes = [raw[c] for c in codes if c < len(raw)]
            members[i] = np.array(codes, np.float32)
        trees.append(dict(feature=np.where(leaf, -1, nd["feature_idx"]).astype(np.int64),
                          threshold=nd["num_threshold"].astype(np.float32),
                          left=nd["left"].astype(np.int64), right=nd["right"].astype(np.int64),
                          mode=["BRANCH_MEMBER" if c else "BRANCH_LEQ" for c in cat],
                          missing_true=nd["missing_go_to_left"].astype(np.int64),
                          leaf_values=vals.astype(np.float32), members=members))
    a = tree_attrs_v5(trees)
    a.update(n_targets=1, aggregate_function=V5_AGGREGATE["SUM"], post_transform=V5_POST["NONE"])
    nodes = [node("TreeEnsemble", [input_name], ["raw" if is_clf else output_name], domain="ai.onnx.ml", **a)]
    if is_clf:
        nodes.append(node("Sigmoid", ["raw"], [output_name]))
    return model(nodes, [value_info(input_name, S.FLOAT, ["N", n_features])],
                 [value_info(output_name, S.FLOAT, ["N", 1])], name="sklearn_hgb", ml_opset=5,
                 metadata={"family": "gbdt", "source": "sklearn"})


def svm(est, n_features: int, scaler=None, output: str = "auto", input_name: str = "input",
        output_name: str = "output"):
    """A fitted binary ``SVC``, ``SVR`` or ``OneClassSVM`` -> ONNX (``SVMClassifier`` / ``SVMRegressor``),
    with an optional fitted ``StandardScaler`` as a ``Scaler`` node in front.

    Reads ``support_vectors_``, the dual coefficients and intercept (``_dual_coef_`` / ``_intercept_``
    for SVC, libsvm's orientation: K @ _dual_coef_ + _intercept_ = -decision_function, positive for
    ``classes_[0]``; ``dual_coef_`` / ``intercept_`` for SVR and OneClassSVM, where it equals
    decision_function), ``_gamma``, ``coef0``, ``degree``, ``n_support_`` and, when the SVC was fitted
    with ``probability=True``, ``probA_`` / ``probB_``. Every number is rounded to float32.

    The model score rises with risk:

    * SVC -> SVMClassifier -> ZipMap: outputs ``label`` [N] and ``output`` [N, 2] in ``classes_``
      order; the score is column 1, P(classes_[1]) by Platt scaling with probabilities, else
      Sigmoid(-dec) (post_transform LOGISTIC);
    * OneClassSVM -> SVMRegressor -> Mul(-1) -> Sigmoid: ``output`` [N, 1], an outlier scores towards 1;
    * SVR -> SVMRegressor: ``output`` [N, 1], the raw value.

    ``output``: "auto" as above; "raw" the bare operator (SVC: scores [dec, -dec] with no post
    transform; OneClassSVM and SVR: dec); "label" OneClassSVM only: one_class = 1, +1 / -1."""
    name = type(est).__name__
    if name not in ("SVC", "SVR", "OneClassSVM"):
        raise ValueError(f"svm: {name} is not converted (SVC, SVR, OneClassSVM)")
    if output not in ("auto", "raw", "label") or (output == "label" and name != "OneClassSVM"):
        raise ValueError(f"svm: output {output!r} for {name}")
    kernel = str(est.kernel).upper()
    if kernel not in ("LINEAR", "POLY", "RBF", "SIGMOID"):
        raise ValueError(f"svm: kernel {est.kernel!r} is not converted")
    sv = np.asarray(est.support_vectors_, np.float32)
    if sv.ndim != 2 or sv.shape[1] != n_features:
        raise ValueError("svm: support vectors do not match n_features (sparse fits are not converted)")
    clf = name == "SVC"
    if clf and len(est.classes_) != 2:
        raise ValueError("only binary classifiers are converted")
    coef = np.asarray(est._dual_coef_ if clf else est.dual_coef_, np.float32).ravel()
    rho = np.asarray(est._intercept_ if clf else est.intercept_, np.float32).ravel()[:1]
    a = dict(kernel_type=kernel, kernel_params=np.array([est._gamma, est.coef0, est.degree], np.float32),
             support_vectors=sv.ravel(), coefficients=coef, rho=rho)
    nodes = []
    x = input_name
    if scaler is not None:
        mean = np.zeros(n_features) if getattr(scaler, "mean_", None) is None else scaler.mean_
        std = np.ones(n_features) if getattr(scaler, "scale_", None) is None else scaler.scale_
        nodes.append(node("Scaler", [x], ["scaled"], domain="ai.onnx.ml", offset=np.asarray(mean, np.float32),
                          scale=(1.0 / np.asarray(std, np.float64)).astype(np.float32)))
        x = "scaled"
    meta = {"family": "svm", "source": "sklearn", "estimator": name}
    ins = [value_info(input_name, S.FLOAT, ["N", n_features])]
    if clf:
        platt = output == "auto" and len(np.ravel(getattr(est, "probA_", []))) == 1
        if platt:
            a.update(prob_a=np.asarray(est.probA_, np.float32).ravel(), prob_b=np.asarray(est.probB_, np.float32).ravel())
        labels = np.asarray(est.classes_)
        ints = labels.dtype.kind in "iub"
        a.update(vectors_per_class=np.asarray(est.n_support_, np.int64),
                 post_transform="LOGISTIC" if output == "auto" and not platt else "NONE")
        lab = (dict(classlabels_ints=labels.astype(np.int64)) if ints
               else dict(classlabels_strings=[str(c) for c in labels]))
        nodes.append(node("SVMClassifier", [x], ["label", "probabilities"], domain="ai.onnx.ml", **a, **lab))
        zl = (dict(classlabels_int64s=labels.astype(np.int64)) if ints else dict(classlabels_strings=lab["classlabels_strings"]))
        nodes.append(node("ZipMap", ["probabilities"], [output_name], domain="ai.onnx.ml", **zl))
        return model(nodes, ins, [value_info("label", S.INT64, ["N"]), value_info(output_name, S.FLOAT, ["N", 2])],
                     name="sklearn_svc", metadata=meta)
    a.update(n_supports=int(sv.shape[0]), post_transform="NONE", one_class=int(output == "label"))
    inits = []
    if name == "OneClassSVM" and output == "auto":
        nodes += [node("SVMRegressor", [x], ["dec"], domain="ai.onnx.ml", **a),
                  node("Mul", ["dec", "minus_one"], ["neg"]), node("Sigmoid", ["neg"], [output_name])]
        inits.append(tensor("minus_one", np.array([-1.0], np.float32)))
    else:
        nodes.append(node("SVMRegressor", [x], [output_name], domain="ai.onnx.ml", **a))
    return model(nodes, ins, [value_info(output_name, S.FLOAT, ["N", 1])], inits,
                 name="sklearn_" + name.lower(), metadata=meta)


_FINAL = {"GradientBoostingClassifier": gradient_boosting, "GradientBoostingRegressor": gradient_boosting,
          "RandomForestRegressor": random_forest, "HistGradientBoostingClassifier": hist_gradient_boosting,
          "HistGradientBoostingRegressor": hist_gradient_boosting, "SVC": svm, "SVR": svm, "OneClassSVM": svm}


def _column_indices(cols, n_features: int, name: str) -> np.ndarray:
    """A ColumnTransformer column specifier (integer list, slice or boolean mask) as indices."""
    if isinstance(cols, (str, bytes)) or callable(cols) or (
            not isinstance(cols, slice) and np.asarray(cols).dtype.kind not in "iub"):
        raise ValueError(f"column_pipeline: columns {cols!r} of {name!r} are not converted (integers, slices, masks)")
    if not isinstance(cols, slice):
        cols = np.asarray(cols)
        if cols.ndim != 1 or (cols.dtype.kind == "b" and cols.size != n_features):
            raise ValueError(f"column_pipeline: columns of {name!r} must be a list of indices or a mask over the input")
    idx = np.arange(n_features)[cols]
    return np.atleast_1d(idx).astype(np.int64)


def column_pipeline(ct, n_features: int, final=None, input_name: str = "input", output_name: str = "output",
                    final_args: Optional[dict] = None):
    """A fitted ``ColumnTransformer`` (optionally with the fitted estimator ``final`` behind it: the two
    halves of ``Pipeline(ct, final)``) -> ONNX.

    Every branch becomes ``ArrayFeatureExtractor`` on the input followed by its transformers:
    ``SimpleImputer`` -> ``Imputer`` (any strategy: the fitted ``statistics_``; ``missing_values`` NaN
    or a number), ``StandardScaler`` -> ``Scaler``, ``MinMaxScaler`` -> ``Scaler`` with offset
    ``-min_ / scale_``, ``OneHotEncoder`` (numeric integral categories, ``handle_unknown="ignore"``,
    ``drop=None``) -> per column ``ArrayFeatureExtractor`` -> ``OneHotEncoder`` -> ``Flatten``, then
    ``Concat``; ``Binarizer``; ``"passthrough"``; a ``Pipeline`` of these. ``"drop"`` branches and a
    dropped remainder emit nothing. The branches meet in one ``Concat`` in the order of
    ``ct.output_indices_``. Constants are rounded to float32.

    ``final``: an estimator :func:`gradient_boosting`, :func:`random_forest`,
    :func:`hist_gradient_boosting` or :func:`svm` converts; its graph reads the assembled value
    (``final_args``: further keyword arguments of that function, such as ``output="raw"``).
    Without it the model's output is the assembled matrix [N, width].

    One difference: scikit-learn's encoder matches a category by equality, the ONNX operator after
    truncation towards zero, so 2.5 matches category 2 here. Integral inputs encode as in sklearn."""
    nodes: List = []
    inits: List = []
    parts: List[str] = []
    width = 0
    count = [0]

    def fresh(stem: str) -> str:
        count[0] += 1
        return f"ct_{stem}_{count[0]}"

    def extract(src: str, idx: np.ndarray) -> str:
        name, out = fresh("idx"), fresh("cols")
        inits.append(tensor(name, np.asarray(idx, np.int64)))
        nodes.append(node("ArrayFeatureExtractor", [src, name], [out], domain="ai.onnx.ml"))
        return out

    def apply(tr, cur: str, k: int, where: str):
        """Append the nodes of one fitted transformer on ``cur`` [N, k]; returns (value, width)."""
        kind = type(tr).__name__
        if isinstance(tr, str):
            if tr == "passthrough":
                return cur, k
            raise ValueError(f"column_pipeline: transformer {tr!r} in {where!r} is not converted")
        if kind == "FunctionTransformer" and tr.func is None:   # how a fitted remainder="passthrough" appears
            return cur, k
        if kind == "Pipeline":
            for _, step in tr.steps:
                cur, k = apply(step, cur, k, where)
            return cur, k
        if kind == "SimpleImputer":
            stats = np.asarray(tr.statistics_, np.float64).ravel()
            if getattr(tr, "add_indicator", False) or stats.size != k or not np.isfinite(stats).all():
                raise ValueError(f"column_pipeline: SimpleImputer in {where!r} (add_indicator, or a column with no "
                                 "observed value) is not converted")
            mv = tr.missing_values
            if not isinstance(mv, (int, float, np.integer, np.floating)) or isinstance(mv, bool):
                raise ValueError(f"column_pipeline: SimpleImputer missing_values {mv!r} in {where!r} (NaN or a number)")
            out = fresh("imputed")
            nodes.append(node("Imputer", [cur], [out], domain="ai.onnx.ml", imputed_value_floats=stats.astype(np.float32),
                              replaced_value_float=float(mv)))
            return out, k
        if kind in ("StandardScaler", "MinMaxScaler"):
            if kind == "StandardScaler":
                off = np.zeros(k) if tr.mean_ is None else np.asarray(tr.mean_, np.float64)
                sc = np.ones(k) if tr.scale_ is None else 1.0 / np.asarray(tr.scale_, np.float64)
            else:
                if getattr(tr, "clip", False):
                    raise ValueError(f"column_pipeline: MinMaxScaler(clip=True) in {where!r} is not converted")
                sc = np.asarray(tr.scale_, np.float64)
                off = -np.asarray(tr.min_, np.float64) / sc
            out = fresh("scaled")
            nodes.append(node("Scaler", [cur], [out], domain="ai.onnx.ml", offset=off.astype(np.float32),
                              scale=sc.astype(np.float32)))
            return out, k
        if kind == "Binarizer":
            out = fresh("binary")
            nodes.append(node("Binarizer", [cur], [out], domain="ai.onnx.ml", threshold=float(tr.threshold)))
            return out, k
        if kind == "OneHotEncoder":
            if tr.handle_unknown != "ignore" or tr.drop is not None or getattr(tr, "min_frequency", None) is not None \
                    or getattr(tr, "max_categories", None) is not None:
                raise ValueError(f"column_pipeline: OneHotEncoder in {where!r} must use handle_unknown='ignore', "
                                 "drop=None and no infrequent categories")
            outs, total = [], 0
            for j, cats in enumerate(tr.categories_):
                c = np.asarray(cats)
                if c.dtype.kind not in "iuf" or not np.isfinite(c.astype(np.float64)).all() \
                        or (c.astype(np.float64) != np.trunc(c.astype(np.float64))).any():
                    raise ValueError(f"column_pipeline: OneHotEncoder in {where!r}: the categories of column {j} are "
                                     "not all integral numbers")
                col, hot, flat = extract(cur, np.array([j])), fresh("onehot"), fresh("hot")
                nodes.append(node("OneHotEncoder", [col], [hot], domain="ai.onnx.ml", cats_int64s=c.astype(np.int64), zeros=1))
                nodes.append(node("Flatten", [hot], [flat], axis=1))
                outs.append(flat)
                total += c.size
            if len(outs) == 1:
                return outs[0], total
            out = fresh("encoded")
            nodes.append(node("Concat", outs, [out], axis=1))
            return out, total
        raise ValueError(f"column_pipeline: transformer {kind} in {where!r} is not converted")

    if type(ct).__name__ != "ColumnTransformer" or not hasattr(ct, "transformers_"):
        raise ValueError("column_pipeline: a fitted ColumnTransformer is required")
    for name, tr, cols in ct.transformers_:
        idx = _column_indices(cols, n_features, name)
        sl = ct.output_indices_[name]
        if (isinstance(tr, str) and tr == "drop") or idx.size == 0:
            if sl.stop != sl.start:
                raise ValueError(f"column_pipeline: branch {name!r} should be empty")
            continue
        cur, k = apply(tr, extract(input_name, idx), int(idx.size), name)
        if (sl.start, sl.stop) != (width, width + k):
            raise ValueError(f"column_pipeline: branch {name!r} lands at columns {width}:{width + k}, "
                             f"scikit-learn puts it at {sl.start}:{sl.stop}")
        parts.append(cur)
        width += k
    if not parts:
        raise ValueError("column_pipeline: the transformer keeps no column")
    assembled = output_name if final is None else "ct_assembled"
    nodes.append(node("Concat", parts, [assembled], axis=1) if len(parts) > 1 else node("Identity", parts, [assembled]))
    ins = [value_info(input_name, S.FLOAT, ["N", n_features])]
    meta = {"family": "columns", "source": "sklearn", "front_end": "ColumnTransformer", "assembled_width": str(width)}
    if final is None:
        return model(nodes, ins, [value_info(output_name, S.FLOAT, ["N", width])], inits, name="sklearn_columns",
                     metadata=meta)
    fname = type(final).__name__
    if fname not in _FINAL:
        raise ValueError(f"column_pipeline: final estimator {fname} is not converted ({', '.join(sorted(_FINAL))})")
    sub = _FINAL[fname](final, width, input_name=assembled, output_name=output_name, **(final_args or {}))
    ml_opset = max([int(o.version) for o in sub.opset_import if o.domain == "ai.onnx.ml"] + [3])
    meta.update({p.key: p.value for p in sub.metadata_props})
    return model(nodes + list(sub.graph.node), ins, list(sub.graph.output), inits + list(sub.graph.initializer),
                 name="sklearn_pipeline", ml_opset=ml_opset, metadata=meta)
