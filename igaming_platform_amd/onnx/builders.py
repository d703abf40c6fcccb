"""Deterministic random-init ONNX models for the five BASELINE configs.

There is no network for trained checkpoints (BASELINE.json: "random-init model weights"),
so each config's model is generated from a fixed seed with the architecture the config
names. Input name ``input`` / primary output ``output`` follow ``onnx_model.go:37-38``.

* cfg1 ``logistic``: input[N,32] -> Gemm -> Sigmoid -> output[N,1]
* cfg2 ``gbdt``:     input[N,128] -> TreeEnsembleClassifier(100 trees, LOGISTIC)
                      -> label[N], output[N,2]
* ``gbdt_v5``:        input[N,32] -> TreeEnsemble (ai.onnx.ml opset 5, a share of BRANCH_MEMBER
                      nodes, LOGISTIC) -> output[N,1]
* cfg3 ``stacked``:  input[N,128] -> TreeEnsembleRegressor(100 trees, n_targets=32)
                      -> Gemm(32x256) -> Relu -> Gemm(256x1) -> Sigmoid -> output[N,1]
* cfg4 ``ltv_mlp``:  input[N,256] -> (Gemm -> Relu) x4 (width 512) -> Gemm -> output[N,1]
* cfg5 ``gru``:      input[T=100,N,16] -> GRU(256) -> Squeeze -> GRU(256) -> Y_h
                      -> Reshape[N,256] -> Gemm -> Sigmoid -> output[N,1]
* ``tcn``:            input[T=100,N,16] -> Transpose[N,16,T] -> residual blocks of dilated causal Conv
                      -> last step / mean / max over time -> Gemm -> Sigmoid -> output[N,1]
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import schema as S
from .writer import ML_DOMAIN, V5_AGGREGATE, V5_POST, model, node, tensor, tree_attrs, tree_attrs_v5, value_info

MODES = ["BRANCH_LEQ", "BRANCH_LT", "BRANCH_GTE", "BRANCH_GT"]


def random_complete_tree(rng: np.random.Generator, depth: int, n_features: int, k: int,
                         leaf_scale: float = 0.1, mixed_modes: bool = False,
                         feature_lo: int = 0) -> Dict[str, np.ndarray]:
    """Complete binary tree in BFS order: node i has children 2i+1 (true) / 2i+2 (false)."""
    n_int = (1 << depth) - 1
    n = (1 << (depth + 1)) - 1
    feature = np.full(n, -1, np.int64)
    feature[:n_int] = rng.integers(feature_lo, n_features, n_int)
    threshold = np.zeros(n, np.float32)
    threshold[:n_int] = rng.uniform(0.05, 0.95, n_int).astype(np.float32)
    left = np.zeros(n, np.int64)
    right = np.zeros(n, np.int64)
    left[:n_int] = 2 * np.arange(n_int) + 1
    right[:n_int] = 2 * np.arange(n_int) + 2
    if mixed_modes:
        mode = [MODES[i] for i in rng.integers(0, 4, n)]
    else:
        mode = ["BRANCH_LEQ"] * n
    missing = rng.integers(0, 2, n).astype(np.int64)
    leaf_values = np.zeros((n, k), np.float32)
    leaf_values[n_int:] = (rng.standard_normal((n - n_int, k)) * leaf_scale).astype(np.float32)
    return dict(feature=feature, threshold=threshold, left=left, right=right, mode=mode,
                missing_true=missing, leaf_values=leaf_values)


def logistic(n_features: int = 32, seed: int = 1):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((n_features, 1)) * 0.5).astype(np.float32)
    b = np.array([-1.0], np.float32)
    nodes = [node("Gemm", ["input", "W", "B"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])], [tensor("W", w), tensor("B", b)],
                 name="fraud_logistic", metadata={"family": "logistic", "features": str(n_features)})


def gbdt(n_trees: int = 100, depth: int = 7, n_features: int = 128, seed: int = 2,
         mixed_modes: bool = False):
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(n_trees):
        t = random_complete_tree(rng, depth, n_features, 1, leaf_scale=0.15, mixed_modes=mixed_modes)
        t["class_offset"] = 1   # weights on class 1 only: ORT's binary case
        trees.append(t)
    a = tree_attrs(trees, "class")
    nodes = [node("TreeEnsembleClassifier", ["input"], ["label", "output"], domain=ML_DOMAIN,
                  post_transform="LOGISTIC", classlabels_int64s=np.array([0, 1], np.int64),
                  base_values=np.array([-0.5], np.float32), **a)]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("label", S.INT64, ["N"]), value_info("output", S.FLOAT, ["N", 2])],
                 name="fraud_gbdt",
                 metadata={"family": "gbdt", "trees": str(n_trees), "depth": str(depth)})


def gbdt_v5(n_trees: int = 50, depth: int = 5, n_features: int = 32, seed: int = 14, member_share: float = 0.3,
            n_categorical: int = 4, categories: int = 40, k: int = 1, post: str = "LOGISTIC"):
    """ai.onnx.ml opset-5 ``TreeEnsemble`` with set-membership splits: random complete trees in
    which about ``member_share`` of the nodes are ``BRANCH_MEMBER`` on one of the first
    ``n_categorical`` columns (category codes 0 .. ``categories`` - 1; every fourth set is shifted
    to negative codes, which the device stores as a value list instead of a bitset). Each leaf
    writes one of the ``k`` targets. Output [N, k], ``post`` applied."""
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(n_trees):
        t = random_complete_tree(rng, depth, n_features, k, leaf_scale=0.15)
        n_int = (1 << depth) - 1
        keep = rng.integers(0, k, len(t["feature"]))  # one target per leaf
        t["leaf_values"] *= (np.arange(k)[None, :] == keep[:, None])
        t["members"] = [None] * len(t["feature"])
        for i in np.flatnonzero(rng.random(n_int) < member_share):
            t["feature"][i] = rng.integers(0, max(1, n_categorical))
            t["mode"][i] = "BRANCH_MEMBER"
            m = rng.choice(categories, size=rng.integers(1, max(2, categories // 2)), replace=False)
            t["members"][i] = (m - categories if rng.integers(0, 4) == 0 else m).astype(np.float32)
        trees.append(t)
    nodes = [node("TreeEnsemble", ["input"], ["output"], domain=ML_DOMAIN, n_targets=k,
                  aggregate_function=V5_AGGREGATE["SUM"], post_transform=V5_POST[post], **tree_attrs_v5(trees))]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", k])], name="fraud_gbdt_v5", ml_opset=5,
                 metadata={"family": "gbdt", "trees": str(n_trees), "depth": str(depth),
                           "member_share": str(member_share)})


def stacked(n_trees: int = 100, depth: int = 7, n_features: int = 128, k: int = 32,
            hidden: int = 256, seed: int = 3):
    rng = np.random.default_rng(seed)
    trees = [random_complete_tree(rng, depth, n_features, k, leaf_scale=0.1) for _ in range(n_trees)]
    a = tree_attrs(trees, "target")
    w1 = (rng.standard_normal((k, hidden)) * np.sqrt(2.0 / k)).astype(np.float32)
    b1 = (rng.standard_normal(hidden) * 0.01).astype(np.float32)
    w2 = (rng.standard_normal((hidden, 1)) * np.sqrt(1.0 / hidden)).astype(np.float32)
    b2 = np.array([-0.25], np.float32)
    nodes = [
        node("TreeEnsembleRegressor", ["input"], ["emb"], domain=ML_DOMAIN, n_targets=k,
             aggregate_function="SUM", post_transform="NONE",
             base_values=np.zeros(k, np.float32), **a),
        node("Gemm", ["emb", "W1", "B1"], ["h1"]),
        node("Relu", ["h1"], ["a1"]),
        node("Gemm", ["a1", "W2", "B2"], ["logit"]),
        node("Sigmoid", ["logit"], ["output"]),
    ]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])],
                 [tensor("W1", w1), tensor("B1", b1), tensor("W2", w2), tensor("B2", b2)],
                 name="fraud_stacked",
                 metadata={"family": "stacked", "trees": str(n_trees), "targets": str(k)})


def ltv_mlp(n_features: int = 256, width: int = 512, layers: int = 4, seed: int = 4):
    rng = np.random.default_rng(seed)
    nodes, inits = [], []
    prev, cur = n_features, "input"
    for i in range(layers):
        w = (rng.standard_normal((prev, width)) * np.sqrt(2.0 / prev)).astype(np.float32)
        b = (rng.standard_normal(width) * 0.01).astype(np.float32)
        inits += [tensor(f"W{i}", w), tensor(f"B{i}", b)]
        nodes += [node("Gemm", [cur, f"W{i}", f"B{i}"], [f"h{i}"]), node("Relu", [f"h{i}"], [f"a{i}"])]
        prev, cur = width, f"a{i}"
    w = (rng.standard_normal((prev, 1)) * np.sqrt(1.0 / prev)).astype(np.float32)
    inits += [tensor("Wout", w), tensor("Bout", np.array([50.0], np.float32))]
    nodes.append(node("Gemm", [cur, "Wout", "Bout"], ["output"]))
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])], inits, name="ltv_mlp",
                 metadata={"family": "mlp", "layers": str(layers), "width": str(width)})


SEQ_LENS = "sequence_lens"   # the graph input gru() / lstm() wire to every layer with seq_lens=True


def _gru_weights(rng, in_dim: int, hidden: int):
    s = 1.0 / np.sqrt(hidden)
    w = rng.uniform(-s, s, (1, 3 * hidden, in_dim)).astype(np.float32)
    r = rng.uniform(-s, s, (1, 3 * hidden, hidden)).astype(np.float32)
    b = rng.uniform(-s, s, (1, 6 * hidden)).astype(np.float32)
    return w, r, b


def gru(seq: int = 100, in_dim: int = 16, hidden: int = 256, seed: int = 5, layers: int = 2,
        linear_before_reset: int = 1, head: bool = True, direction: str = "forward", layout: int = 0,
        seq_lens: bool = False):
    """GRU sequence classifier. ``direction`` forward / reverse / bidirectional (one layer),
    ``layout`` 0 ([seq, N, in]) or 1 (batch-major [N, seq, in]). ``seq_lens``: a second graph
    input ``sequence_lens`` (int32 [N]) wired to every layer, as a model trained on packed or padded
    sequences exports."""
    rng = np.random.default_rng(seed)
    D = 2 if direction == "bidirectional" else 1
    if D == 2 and layers != 1:
        raise ValueError("bidirectional: one layer")

    def weights(i):
        ws = [_gru_weights(rng, i, hidden) for _ in range(D)]
        return tuple(np.concatenate([w[k] for w in ws], 0) for k in range(3))
    w1, r1, b1 = weights(in_dim)
    wh = (rng.standard_normal((D * hidden, 1)) * np.sqrt(1.0 / (D * hidden))).astype(np.float32)
    bh = np.array([0.0], np.float32)
    lbr = int(linear_before_reset)
    attrs = dict(hidden_size=hidden, linear_before_reset=lbr)
    if direction != "forward":
        attrs["direction"] = direction
    if layout:
        attrs["layout"] = int(layout)
    lens = [SEQ_LENS] if seq_lens else []
    nodes = [node("GRU", ["input", "W1", "R1", "B1"] + lens, ["Y1", "Yh1"], **attrs)]
    # Y: layout 0 [seq, D, N, H] -> squeeze axis 1; layout 1 [N, seq, D, H] -> squeeze axis 2
    inits = [tensor("W1", w1), tensor("R1", r1), tensor("B1", b1),
             tensor("ax1", np.array([2 if layout else 1], np.int64)),
             tensor("shp", np.array([-1, D * hidden], np.int64))]
    last_h = "Yh1"
    if layers == 2:
        w2, r2, b2 = weights(hidden)
        nodes += [node("Squeeze", ["Y1", "ax1"], ["X2"]),
                  node("GRU", ["X2", "W2", "R2", "B2"] + lens, ["Y2", "Yh2"], **attrs)]
        inits += [tensor("W2", w2), tensor("R2", r2), tensor("B2", b2)]
        last_h = "Yh2"
    if D == 2 and not layout:  # Y_h [2, N, H] -> [N, 2, H] -> [N, 2H]
        nodes.append(node("Transpose", [last_h], ["hT"], perm=[1, 0, 2]))
        last_h = "hT"
    if head:
        nodes += [node("Reshape", [last_h, "shp"], ["h"]), node("Gemm", ["h", "Wh", "Bh"], ["logit"]),
                  node("Sigmoid", ["logit"], ["output"])]
        inits += [tensor("Wh", wh), tensor("Bh", bh)]
        out_vi = value_info("output", S.FLOAT, ["N", 1])
    else:
        nodes.append(node("Reshape", [last_h, "shp"], ["output"]))
        out_vi = value_info("output", S.FLOAT, ["N", D * hidden])
    x_dims = ["N", seq, in_dim] if layout else [seq, "N", in_dim]
    in_vis = [value_info("input", S.FLOAT, x_dims)] + ([value_info(SEQ_LENS, S.INT32, ["N"])] if seq_lens else [])
    return model(nodes, in_vis, [out_vi], inits, name="abuse_gru",
                 metadata={"family": "gru", "layers": str(layers), "hidden": str(hidden), "seq": str(seq),
                           "direction": direction, "layout": str(layout)})


def _lstm_weights(rng, in_dim: int, hidden: int):
    s = 1.0 / np.sqrt(hidden)
    w = rng.uniform(-s, s, (1, 4 * hidden, in_dim)).astype(np.float32)
    r = rng.uniform(-s, s, (1, 4 * hidden, hidden)).astype(np.float32)
    b = rng.uniform(-s, s, (1, 8 * hidden)).astype(np.float32)
    return w, r, b


def lstm(seq: int = 100, in_dim: int = 16, hidden: int = 256, seed: int = 11, layers: int = 2,
         head: bool = True, direction: str = "forward", layout: int = 0, seq_lens: bool = False):
    """LSTM sequence classifier (ONNX gate order i, o, f, c), built like :func:`gru`: ``direction``
    forward / reverse / bidirectional (one layer), ``layout`` 0 ([seq, N, in]) or 1 ([N, seq, in]),
    ``seq_lens`` the ``sequence_lens`` graph input."""
    rng = np.random.default_rng(seed)
    D = 2 if direction == "bidirectional" else 1
    if D == 2 and layers != 1:
        raise ValueError("bidirectional: one layer")

    def weights(i):
        ws = [_lstm_weights(rng, i, hidden) for _ in range(D)]
        return tuple(np.concatenate([w[k] for w in ws], 0) for k in range(3))
    w1, r1, b1 = weights(in_dim)
    wh = (rng.standard_normal((D * hidden, 1)) * np.sqrt(1.0 / (D * hidden))).astype(np.float32)
    bh = np.array([0.0], np.float32)
    attrs = dict(hidden_size=hidden)
    if direction != "forward":
        attrs["direction"] = direction
    if layout:
        attrs["layout"] = int(layout)
    lens = [SEQ_LENS] if seq_lens else []
    nodes = [node("LSTM", ["input", "W1", "R1", "B1"] + lens, ["Y1", "Yh1"], **attrs)]
    # Y: layout 0 [seq, D, N, H] -> squeeze axis 1; layout 1 [N, seq, D, H] -> squeeze axis 2
    inits = [tensor("W1", w1), tensor("R1", r1), tensor("B1", b1),
             tensor("ax1", np.array([2 if layout else 1], np.int64)),
             tensor("shp", np.array([-1, D * hidden], np.int64))]
    last_h = "Yh1"
    if layers == 2:
        w2, r2, b2 = weights(hidden)
        nodes += [node("Squeeze", ["Y1", "ax1"], ["X2"]),
                  node("LSTM", ["X2", "W2", "R2", "B2"] + lens, ["Y2", "Yh2"], **attrs)]
        inits += [tensor("W2", w2), tensor("R2", r2), tensor("B2", b2)]
        last_h = "Yh2"
    if D == 2 and not layout:  # Y_h [2, N, H] -> [N, 2, H] -> [N, 2H]
        nodes.append(node("Transpose", [last_h], ["hT"], perm=[1, 0, 2]))
        last_h = "hT"
    if head:
        nodes += [node("Reshape", [last_h, "shp"], ["h"]), node("Gemm", ["h", "Wh", "Bh"], ["logit"]),
                  node("Sigmoid", ["logit"], ["output"])]
        inits += [tensor("Wh", wh), tensor("Bh", bh)]
        out_vi = value_info("output", S.FLOAT, ["N", 1])
    else:
        nodes.append(node("Reshape", [last_h, "shp"], ["output"]))
        out_vi = value_info("output", S.FLOAT, ["N", D * hidden])
    x_dims = ["N", seq, in_dim] if layout else [seq, "N", in_dim]
    in_vis = [value_info("input", S.FLOAT, x_dims)] + ([value_info(SEQ_LENS, S.INT32, ["N"])] if seq_lens else [])
    return model(nodes, in_vis, [out_vi], inits, name="abuse_lstm",
                 metadata={"family": "lstm", "layers": str(layers), "hidden": str(hidden), "seq": str(seq),
                           "direction": direction, "layout": str(layout)})


def _scaler(rng, n_features: int):
    """sklearn StandardScaler as ai.onnx.ml Scaler: (x - mean) * (1 / std)."""
    mean = rng.uniform(-0.5, 0.5, n_features).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, n_features).astype(np.float32)
    return node("Scaler", ["input"], ["scaled"], domain=ML_DOMAIN, offset=mean, scale=scale)


def sklearn_linear(n_features: int = 32, classes: int = 2, post: str = "LOGISTIC", seed: int = 6,
                   scaler: bool = True, zipmap: bool = True, string_labels: bool = False):
    """sklearn-onnx style linear pipeline: [Scaler] -> LinearClassifier -> [ZipMap].
    ``classes`` 2 writes one coefficient row (sklearn's binary LogisticRegression); more write
    one row per class."""
    rng = np.random.default_rng(seed)
    E = 1 if classes == 2 else classes
    coef = (rng.standard_normal((E, n_features)) * 0.3).astype(np.float32)
    icpt = (rng.standard_normal(E) * 0.1).astype(np.float32)
    labels = (dict(classlabels_strings=[f"c{i}" for i in range(classes)]) if string_labels
              else dict(classlabels_ints=np.arange(classes, dtype=np.int64)))
    nodes = [_scaler(rng, n_features)] if scaler else []
    x = "scaled" if scaler else "input"
    probs = "probabilities" if zipmap else "output"
    nodes.append(node("LinearClassifier", [x], ["label", probs], domain=ML_DOMAIN, coefficients=coef.ravel(),
                      intercepts=icpt, post_transform=post, multi_class=0, **labels))
    if zipmap:
        zl = (dict(classlabels_strings=labels["classlabels_strings"]) if string_labels
              else dict(classlabels_int64s=np.arange(classes, dtype=np.int64)))
        nodes.append(node("ZipMap", [probs], ["output"], domain=ML_DOMAIN, **zl))
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("label", S.INT64, ["N"]), value_info("output", S.FLOAT, ["N", classes])],
                 name="sklearn_linear", metadata={"family": "linear", "classes": str(classes)})


def linear_regressor(n_features: int = 32, targets: int = 1, post: str = "NONE", seed: int = 7):
    rng = np.random.default_rng(seed)
    coef = (rng.standard_normal((targets, n_features)) * 0.3).astype(np.float32)
    icpt = (rng.standard_normal(targets) * 0.1).astype(np.float32)
    nodes = [_scaler(rng, n_features),
             node("LinearRegressor", ["scaled"], ["output"], domain=ML_DOMAIN, coefficients=coef.ravel(),
                  intercepts=icpt, targets=targets, post_transform=post)]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", targets])], name="linear_regressor",
                 metadata={"family": "linear"})


def mlp_classifier(n_features: int = 32, hidden: int = 64, seed: int = 8):
    """sklearn MLPClassifier-style pipeline: Scaler -> Gemm -> Relu -> LinearClassifier (binary,
    LOGISTIC) -> ZipMap. On the device: the Scaler folds into the first layer's weights and the
    two layers run as one fused head."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((n_features, hidden)) * np.sqrt(2.0 / n_features)).astype(np.float32)
    b = (rng.standard_normal(hidden) * 0.01).astype(np.float32)
    coef = (rng.standard_normal(hidden) * np.sqrt(1.0 / hidden)).astype(np.float32)
    nodes = [_scaler(rng, n_features), node("Gemm", ["scaled", "W", "B"], ["h"]), node("Relu", ["h"], ["a"]),
             node("LinearClassifier", ["a"], ["label", "probabilities"], domain=ML_DOMAIN, coefficients=coef,
                  intercepts=np.array([-0.1], np.float32), post_transform="LOGISTIC",
                  classlabels_ints=np.array([0, 1], np.int64)),
             node("ZipMap", ["probabilities"], ["output"], domain=ML_DOMAIN,
                  classlabels_int64s=np.array([0, 1], np.int64))]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("label", S.INT64, ["N"]), value_info("output", S.FLOAT, ["N", 2])],
                 [tensor("W", w), tensor("B", b)], name="mlp_classifier", metadata={"family": "mlp"})


def wide_deep(n_features: int = 32, hidden: int = 128, deep_out: int = 64, wide: int = 16, seed: int = 9):
    """DAG: a deep tower (Gemm -> Relu -> Gemm -> Relu) and a wide linear branch read the same
    input; Concat -> Gemm -> Sigmoid."""
    rng = np.random.default_rng(seed)

    def lin(k, n, name):
        return [tensor(f"W{name}", (rng.standard_normal((k, n)) * np.sqrt(2.0 / k)).astype(np.float32)),
                tensor(f"B{name}", (rng.standard_normal(n) * 0.01).astype(np.float32))]
    inits = lin(n_features, hidden, "d1") + lin(hidden, deep_out, "d2") + lin(n_features, wide, "w") + \
        lin(deep_out + wide, 1, "o")
    nodes = [node("Gemm", ["input", "Wd1", "Bd1"], ["d1"]), node("Relu", ["d1"], ["a1"]),
             node("Gemm", ["a1", "Wd2", "Bd2"], ["d2"]), node("Relu", ["d2"], ["a2"]),
             node("Gemm", ["input", "Ww", "Bw"], ["wide"]),
             node("Concat", ["a2", "wide"], ["cat"], axis=1),
             node("Gemm", ["cat", "Wo", "Bo"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])], inits, name="wide_deep", metadata={"family": "mlp"})


def residual_mlp(n_features: int = 32, width: int = 128, blocks: int = 2, seed: int = 10):
    """DAG: h = Relu(x W0 + b0); per block h = h + Relu(Relu(h W1 + b1) W2 + b2) (MatMul + Add
    pairs); head Gemm -> Sigmoid."""
    rng = np.random.default_rng(seed)
    inits = [tensor("W0", (rng.standard_normal((n_features, width)) * np.sqrt(2.0 / n_features)).astype(np.float32)),
             tensor("B0", np.zeros(width, np.float32))]
    nodes = [node("Gemm", ["input", "W0", "B0"], ["z0"]), node("Relu", ["z0"], ["h0"])]
    h = "h0"
    for i in range(blocks):
        for j in (1, 2):
            inits += [tensor(f"W{i}_{j}", (rng.standard_normal((width, width)) * np.sqrt(1.0 / width)).astype(np.float32)),
                      tensor(f"B{i}_{j}", (rng.standard_normal(width) * 0.01).astype(np.float32))]
        nodes += [node("MatMul", [h, f"W{i}_1"], [f"m{i}_1"]), node("Add", [f"m{i}_1", f"B{i}_1"], [f"z{i}_1"]),
                  node("Relu", [f"z{i}_1"], [f"a{i}_1"]),
                  node("MatMul", [f"a{i}_1", f"W{i}_2"], [f"m{i}_2"]), node("Add", [f"m{i}_2", f"B{i}_2"], [f"z{i}_2"]),
                  node("Relu", [f"z{i}_2"], [f"a{i}_2"]),
                  node("Add", [h, f"a{i}_2"], [f"h{i + 1}"])]
        h = f"h{i + 1}"
    inits += [tensor("Wh", (rng.standard_normal((width, 1)) * np.sqrt(1.0 / width)).astype(np.float32)),
              tensor("Bh", np.array([-0.2], np.float32))]
    nodes += [node("Gemm", [h, "Wh", "Bh"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])], inits, name="residual_mlp", metadata={"family": "mlp"})


def _torch_linear(rng, k: int, n: int, name: str, gain: float = 2.0):
    """torch.nn.Linear as the exporter writes it: Gemm(transB=1) on a [out, in] weight."""
    return [tensor(f"W{name}", (rng.standard_normal((n, k)) * np.sqrt(gain / k)).astype(np.float32)),
            tensor(f"B{name}", (rng.standard_normal(n) * 0.01).astype(np.float32))]


def _batch_norm(rng, width: int, x: str, y: str, name: str):
    """nn.BatchNorm1d in eval mode: per-column scale / B and running mean / var initializers."""
    inits = [tensor(f"bn{name}_s", rng.uniform(0.5, 1.5, width).astype(np.float32)),
             tensor(f"bn{name}_b", (rng.standard_normal(width) * 0.1).astype(np.float32)),
             tensor(f"bn{name}_m", (rng.standard_normal(width) * 0.2).astype(np.float32)),
             tensor(f"bn{name}_v", rng.uniform(0.5, 2.0, width).astype(np.float32))]
    return node("BatchNormalization", [x] + [t.name for t in inits], [y], epsilon=1e-5), inits


def _layer_norm(rng, width: int, x: str, y: str, name: str):
    inits = [tensor(f"ln{name}_s", rng.uniform(0.5, 1.5, width).astype(np.float32)),
             tensor(f"ln{name}_b", (rng.standard_normal(width) * 0.1).astype(np.float32))]
    return node("LayerNormalization", [x] + [t.name for t in inits], [y], axis=-1, epsilon=1e-5), inits


def torch_mlp(n_features: int = 32, hidden: int = 64, layers: int = 2, act: str = "Relu", out: int = 2,
              seed: int = 12):
    """An MLP as torch.onnx exports it: (Gemm -> BatchNormalization -> ``act`` -> Dropout) x
    ``layers``, then Gemm(.., 2) -> Softmax (``out`` 2) or Gemm(.., 1) -> Sigmoid (``out`` 1).
    ``act`` is the ONNX op: Relu, Sigmoid, Tanh, LeakyRelu, Elu, Selu, Softplus, HardSigmoid, Gelu
    or PRelu (one slope per column)."""
    if out not in (1, 2):
        raise ValueError("out: 1 (Sigmoid) or 2 (Softmax)")
    rng = np.random.default_rng(seed)
    nodes, inits = [], [tensor("ratio", np.array(0.1, np.float32))]
    prev, cur = n_features, "input"
    for i in range(layers):
        inits += _torch_linear(rng, prev, hidden, str(i))
        bn, bn_inits = _batch_norm(rng, hidden, f"z{i}", f"n{i}", str(i))
        inits += bn_inits
        a_in = [f"n{i}"]
        if act == "PRelu":
            inits.append(tensor(f"slope{i}", rng.uniform(0.05, 0.3, hidden).astype(np.float32)))
            a_in.append(f"slope{i}")
        nodes += [node("Gemm", [cur, f"W{i}", f"B{i}"], [f"z{i}"], transB=1), bn, node(act, a_in, [f"a{i}"]),
                  node("Dropout", [f"a{i}", "ratio"], [f"d{i}"])]
        prev, cur = hidden, f"d{i}"
    inits += _torch_linear(rng, prev, out, "o", gain=1.0)
    nodes += [node("Gemm", [cur, "Wo", "Bo"], ["logits"], transB=1),
              node("Softmax", ["logits"], ["output"], axis=1) if out == 2 else node("Sigmoid", ["logits"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", out])], inits, name="torch_mlp",
                 metadata={"family": "mlp", "layers": str(layers), "act": act})


def tabular_resnet(n_features: int = 32, width: int = 128, blocks: int = 2, norm: str = "layer", seed: int = 13):
    """The ResNet-style tabular MLP: Gemm; per block norm -> Gemm -> Relu -> Dropout -> Gemm ->
    Dropout -> Add(skip) -> Relu; then norm -> Relu -> Gemm -> Sigmoid. ``norm``: layer
    (LayerNormalization) or batch (BatchNormalization)."""
    if norm not in ("layer", "batch"):
        raise ValueError("norm: layer or batch")
    rng = np.random.default_rng(seed)
    mk = _layer_norm if norm == "layer" else _batch_norm
    inits = _torch_linear(rng, n_features, width, "in")
    nodes = [node("Gemm", ["input", "Win", "Bin"], ["h0"], transB=1)]
    h = "h0"
    for i in range(blocks):
        nrm, n_inits = mk(rng, width, h, f"n{i}", str(i))
        inits += n_inits + _torch_linear(rng, width, width, f"{i}_1") + _torch_linear(rng, width, width, f"{i}_2", 1.0)
        nodes += [nrm, node("Gemm", [f"n{i}", f"W{i}_1", f"B{i}_1"], [f"z{i}_1"], transB=1),
                  node("Relu", [f"z{i}_1"], [f"a{i}_1"]), node("Dropout", [f"a{i}_1"], [f"d{i}_1"]),
                  node("Gemm", [f"d{i}_1", f"W{i}_2", f"B{i}_2"], [f"z{i}_2"], transB=1),
                  node("Dropout", [f"z{i}_2"], [f"d{i}_2"]),
                  node("Add", [h, f"d{i}_2"], [f"s{i}"]), node("Relu", [f"s{i}"], [f"h{i + 1}"])]
        h = f"h{i + 1}"
    nrm, n_inits = mk(rng, width, h, "nf", "f")
    inits += n_inits + _torch_linear(rng, width, 1, "o", 1.0)
    nodes += [nrm, node("Relu", ["nf"], ["af"]), node("Gemm", ["af", "Wo", "Bo"], ["logit"], transB=1),
              node("Sigmoid", ["logit"], ["output"])]
    return model(nodes, [value_info("input", S.FLOAT, ["N", n_features])],
                 [value_info("output", S.FLOAT, ["N", 1])], inits, name="tabular_resnet",
                 metadata={"family": "mlp", "blocks": str(blocks), "norm": norm})


def _qparams(lo: float, hi: float, int8: bool, pow2: bool):
    """(scale, zero point) of an asymmetric 8-bit range that holds [lo, hi] and zero, as ORT's static
    quantiser derives them from calibration; ``pow2`` rounds the scale to a power of two."""
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    qmin, qmax = (-128, 127) if int8 else (0, 255)
    scale = max(hi - lo, 1e-6) / (qmax - qmin)
    if pow2:
        scale = 2.0 ** round(np.log2(scale))
    zp = int(np.clip(np.rint(qmin - lo / scale), qmin, qmax))
    return np.float32(scale), zp


def qdq_mlp(widths=(30, 64, 1), seed: int = 15, act_int8: bool = False, per_channel: bool = False,
            bias: str = "int32", pow2: bool = False, w_uint8: bool = False, out_qdq: bool = False,
            hidden_act: str = "Relu", transB: bool = False, opset: int = 13, calib_rows: int = 512,
            clip: float = 0.97, family: str = "mlp"):
    """A random float MLP quantised the way ORT's static quantiser writes it (QDQ format):

        input -> Q -> DQ -> Gemm(DQ(W), DQ(b)) -> ``hidden_act`` -> Q -> DQ -> ... -> Gemm -> Sigmoid

    ``widths``: input, hidden ..., output (1). Activations are uint8 (``act_int8``: int8), weights
    int8 with zero point 0, per tensor or per output channel (``per_channel``; ``w_uint8``: uint8
    with zero point 128). ``bias``: ``int32`` (quantised, through DequantizeLinear), ``float`` (a
    float initializer) or ``add`` (MatMul + Add of the dequantised int32 bias). ``transB`` stores
    the weights [N, K]. ``pow2`` rounds every scale to a power of two (all arithmetic is then
    exact in f32). ``out_qdq`` appends a Q -> DQ pair to the output. ``opset`` 10 writes the
    attribute-free per-tensor form. Activation ranges come from a calibration pass over random
    inputs: each range covers the ``clip`` quantile, so a few per cent of the values saturate."""
    if bias not in ("int32", "float", "add"):
        raise ValueError("bias: int32, float or add")
    if opset < 13 and per_channel:
        raise ValueError("per-channel scales need the opset-13 axis attribute")
    if bias == "add" and transB:
        raise ValueError("MatMul has no transB")
    rng = np.random.default_rng(seed)
    widths = [int(w) for w in widths]
    ws = [(rng.standard_normal((k, n)) * np.sqrt(2.0 / k)).astype(np.float32) for k, n in zip(widths, widths[1:])]
    bs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in widths[1:]]
    calib = rng.uniform(-1.0, 2.0, (calib_rows, widths[0])).astype(np.float32)
    zp_dt = np.int8 if act_int8 else np.uint8
    nodes, inits = [], []

    def act_q(x: str, name: str, h: np.ndarray):
        """Q -> DQ on ``x`` with the range of the calibration values ``h``; returns the DQ output."""
        s, z = _qparams(np.quantile(h, 1.0 - clip), np.quantile(h, clip), act_int8, pow2)
        inits.extend([tensor(f"{name}_scale", np.array(s, np.float32)), tensor(f"{name}_zp", np.array(z, zp_dt))])
        nodes.extend([node("QuantizeLinear", [x, f"{name}_scale", f"{name}_zp"], [f"{name}_q"]),
                      node("DequantizeLinear", [f"{name}_q", f"{name}_scale", f"{name}_zp"], [f"{name}_dq"])])
        q = np.clip(np.rint(h / s) + z, *((-128, 127) if act_int8 else (0, 255)))
        return f"{name}_dq", s, ((q - z) * s).astype(np.float32)

    cur, s_x, h = act_q("input", "x0", calib)
    for i, (w, b) in enumerate(zip(ws, bs)):
        last = i == len(ws) - 1
        amax = np.abs(w).max(axis=0 if per_channel else None)
        s_w = np.maximum(amax, 1e-6) / 127.0
        if pow2:
            s_w = 2.0 ** np.ceil(np.log2(s_w))
        s_w = np.asarray(s_w, np.float32)
        wq = np.clip(np.rint(w / s_w), -127, 127).astype(np.int64)          # [K, N]
        w_dq = (wq * s_w).astype(np.float32)
        z_w = 128 if w_uint8 else 0
        w_store = (wq + z_w).astype(np.uint8 if w_uint8 else np.int8)
        axis = 1
        if transB:
            w_store, axis = np.ascontiguousarray(w_store.T), 0
        ax = dict(axis=axis) if per_channel else {}
        inits.extend([tensor(f"W{i}_q", w_store), tensor(f"W{i}_scale", s_w),
                      tensor(f"W{i}_zp", np.full(s_w.shape, z_w, w_store.dtype))])
        nodes.append(node("DequantizeLinear", [f"W{i}_q", f"W{i}_scale", f"W{i}_zp"], [f"W{i}_dq"], **ax))
        b_dq = b
        if bias != "float":
            s_b = (np.float64(s_x) * s_w.astype(np.float64)).astype(np.float32)
            bq = np.rint(b / s_b).astype(np.int32)
            b_dq = (bq * s_b.astype(np.float64)).astype(np.float32)
            s_b = np.broadcast_to(s_b, (widths[i + 1],)) if per_channel else s_b
            inits.extend([tensor(f"B{i}_q", bq), tensor(f"B{i}_scale", np.ascontiguousarray(s_b, np.float32))])
            nodes.append(node("DequantizeLinear", [f"B{i}_q", f"B{i}_scale"], [f"B{i}_dq"],
                              **(dict(axis=0) if per_channel else {})))
        else:
            inits.append(tensor(f"B{i}_dq", b))
        if bias == "add":
            nodes.extend([node("MatMul", [cur, f"W{i}_dq"], [f"m{i}"]), node("Add", [f"m{i}", f"B{i}_dq"], [f"z{i}"])])
        else:
            nodes.append(node("Gemm", [cur, f"W{i}_dq", f"B{i}_dq"], [f"z{i}"], **(dict(transB=1) if transB else {})))
        z = h.astype(np.float64) @ w_dq.astype(np.float64) + b_dq
        if last:
            nodes.append(node("Sigmoid", [f"z{i}"], ["prob" if out_qdq else "output"]))
            h = 1.0 / (1.0 + np.exp(-z))
        else:
            attrs = dict(alpha=0.125) if hidden_act == "LeakyRelu" else {}
            nodes.append(node(hidden_act, [f"z{i}"], [f"a{i}"], **attrs))
            h = {"Relu": lambda v: np.maximum(v, 0), "LeakyRelu": lambda v: np.where(v > 0, v, 0.125 * v),
                 "Tanh": np.tanh, "Sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v))}[hidden_act](z).astype(np.float32)
            cur, s_x, h = act_q(f"a{i}", f"x{i + 1}", h)
    if out_qdq:
        s, z = (np.float32(2.0 ** -8), -128 if act_int8 else 0)
        inits.extend([tensor("out_scale", np.array(s, np.float32)), tensor("out_zp", np.array(z, zp_dt))])
        nodes.extend([node("QuantizeLinear", ["prob", "out_scale", "out_zp"], ["out_q"]),
                      node("DequantizeLinear", ["out_q", "out_scale", "out_zp"], ["output"])])
    return model(nodes, [value_info("input", S.FLOAT, ["N", widths[0]])],
                 [value_info("output", S.FLOAT, ["N", widths[-1]])], inits, name="qdq_mlp", opset=opset,
                 metadata={"family": family, "format": "qdq", "layers": str(len(ws))})


def svm(n_features: int = 30, n_sv: int = 100, kernel: str = "RBF", op: str = "regressor", seed: int = 16,
        gamma: float = None, coef0: float = 0.5, degree: float = 3.0, one_class: bool = False, platt: bool = False,
        post: str = "NONE", scaler: bool = False, integer: bool = False, tail: str = "none"):
    """A random kernel machine, no fit: ``op`` "regressor" (SVMRegressor -> output [N, 1]) or
    "classifier" (two-class SVMClassifier -> label [N], output [N, 2], optionally Platt-scaled).
    ``integer``: small-integer support vectors and coefficients (with integer ``gamma`` / ``coef0``
    the LINEAR and POLY values are exact in float32). ``tail`` "neg_sigmoid" appends Mul(-1) ->
    Sigmoid to a regressor (the one-class risk score)."""
    rng = np.random.default_rng(seed)
    if integer:
        sv = rng.integers(-3, 4, (n_sv, n_features)).astype(np.float32)
        coef = rng.integers(-2, 3, n_sv).astype(np.float32)
        rho = np.array([float(rng.integers(-2, 3))], np.float32)
    else:
        sv = rng.standard_normal((n_sv, n_features)).astype(np.float32)
        coef = (rng.standard_normal(n_sv) * 0.5).astype(np.float32)
        rho = (rng.standard_normal(1) * 0.1).astype(np.float32)
    g = 1.0 / n_features if gamma is None else gamma
    a = dict(kernel_type=kernel, kernel_params=np.array([g, coef0, degree], np.float32), support_vectors=sv.ravel(),
             coefficients=coef, rho=rho, post_transform=post)
    nodes = [_scaler(rng, n_features)] if scaler else []
    x = "scaled" if scaler else "input"
    ins = [value_info("input", S.FLOAT, ["N", n_features])]
    meta = {"family": "svm", "kernel": kernel}
    if op == "classifier":
        n0 = max(1, n_sv // 2) if n_sv > 1 else 1
        a.update(vectors_per_class=np.array([n0, n_sv - n0], np.int64), classlabels_ints=np.array([0, 1], np.int64))
        if platt:
            a.update(prob_a=np.array([-1.5], np.float32), prob_b=np.array([0.25], np.float32))
        nodes.append(node("SVMClassifier", [x], ["label", "probabilities"], domain=ML_DOMAIN, **a))
        nodes.append(node("ZipMap", ["probabilities"], ["output"], domain=ML_DOMAIN,
                          classlabels_int64s=np.array([0, 1], np.int64)))
        return model(nodes, ins, [value_info("label", S.INT64, ["N"]), value_info("output", S.FLOAT, ["N", 2])],
                     name="svm_classifier", metadata=meta)
    a.update(n_supports=n_sv, one_class=int(one_class))
    inits = []
    if tail == "neg_sigmoid":
        nodes += [node("SVMRegressor", [x], ["dec"], domain=ML_DOMAIN, **a), node("Mul", ["dec", "minus_one"], ["neg"]),
                  node("Sigmoid", ["neg"], ["output"])]
        inits.append(tensor("minus_one", np.array([-1.0], np.float32)))
    else:
        nodes.append(node("SVMRegressor", [x], ["output"], domain=ML_DOMAIN, **a))
    return model(nodes, ins, [value_info("output", S.FLOAT, ["N", 1])], inits, name="svm_regressor", metadata=meta)


def columns(n_features: int = 30, n_trees: int = 20, depth: int = 4, seed: int = 18, final: str = "gbdt"):
    """A random column program (what a scikit-learn ColumnTransformer exports to) in front of a small
    GBDT: over a random permutation of the input columns,

    * ~40 % numeric: Slice -> Imputer(NaN -> a constant per column) -> Scaler;
    * two sentinel columns: Gather -> Imputer(replaced -999);
    * two categorical columns, one through ArrayFeatureExtractor -> Cast(int64) -> OneHotEncoder ->
      Flatten, one through a scalar-index Gather ([N]) -> OneHotEncoder ([N, n_cats]), with negative
      categories;
    * three flags: ArrayFeatureExtractor -> Binarizer;
    * the rest passed through in reverse order (Slice with step -1);

    joined by one Concat, then TreeEnsembleRegressor -> Sigmoid -> output [N, 1]. ``final`` "none"
    ends at the assembled matrix instead (output [N, width]), "dense" at Gemm(width -> 8) -> Relu
    (output [N, 8]). The input is first permuted by an
    ArrayFeatureExtractor, so every branch selects from a view, not from the input itself."""
    if n_features < 12:
        raise ValueError("columns: at least 12 input columns")
    rng = np.random.default_rng(seed)
    nodes, inits = [], []

    def const(name, arr):
        inits.append(tensor(name, arr))
        return name

    perm = rng.permutation(n_features).astype(np.int64)
    nodes.append(node("ArrayFeatureExtractor", ["input", const("perm", perm)], ["p"], domain=ML_DOMAIN))
    n_num = max(2, int(0.4 * n_features))
    # numeric: p[:, :n_num]
    nodes.append(node("Slice", ["p", const("num_s", np.array([0], np.int64)), const("num_e", np.array([n_num], np.int64)),
                                const("ax1", np.array([1], np.int64))], ["num"]))
    nodes.append(node("Imputer", ["num"], ["num_i"], domain=ML_DOMAIN, replaced_value_float=float("nan"),
                      imputed_value_floats=rng.uniform(0.2, 0.8, n_num).astype(np.float32)))
    nodes.append(node("Scaler", ["num_i"], ["num_s_out"], domain=ML_DOMAIN,
                      offset=rng.uniform(0.3, 0.7, n_num).astype(np.float32),
                      scale=rng.uniform(0.5, 4.0, n_num).astype(np.float32)))
    c = n_num
    # sentinel columns
    nodes.append(node("Gather", ["p", const("sen_idx", np.array([c, c + 1], np.int32))], ["sen"], axis=1))
    nodes.append(node("Imputer", ["sen"], ["sen_i"], domain=ML_DOMAIN, replaced_value_float=-999.0,
                      imputed_value_floats=np.array([0.5], np.float32)))
    c += 2
    # categorical: Cast + OneHotEncoder on [N, 1]; a scalar Gather + OneHotEncoder on [N]
    cats_a = np.arange(-2, 4, dtype=np.int64)
    cats_b = np.array([0, 1, 2, 3, 5, 8, 13], np.int64)
    nodes.append(node("ArrayFeatureExtractor", ["p", const("cat_a_idx", np.array([c], np.int64))], ["cat_a"], domain=ML_DOMAIN))
    nodes.append(node("Cast", ["cat_a"], ["cat_a_int"], to=S.INT64))
    nodes.append(node("OneHotEncoder", ["cat_a_int"], ["hot_a3"], domain=ML_DOMAIN, cats_int64s=cats_a, zeros=1))
    nodes.append(node("Flatten", ["hot_a3"], ["hot_a"], axis=1))
    scalar = tensor("cat_b_idx", np.array([c + 1 - n_features], np.int64))
    del scalar.dims[:]   # rank 0: the Gather drops the axis
    inits.append(scalar)
    nodes.append(node("Gather", ["p", "cat_b_idx"], ["cat_b"], axis=-1))
    nodes.append(node("OneHotEncoder", ["cat_b"], ["hot_b"], domain=ML_DOMAIN, cats_int64s=cats_b))
    c += 2
    # flags
    nodes.append(node("ArrayFeatureExtractor", ["p", const("flag_idx", np.array([c, c + 1, c + 2], np.int64))], ["flag"],
                      domain=ML_DOMAIN))
    nodes.append(node("Binarizer", ["flag"], ["flag_b"], domain=ML_DOMAIN, threshold=0.5))
    c += 3
    # the rest, last column first: p[:, -1 : c - 1 : -1]
    nodes.append(node("Slice", ["p", const("rest_s", np.array([-1], np.int64)),
                                const("rest_e", np.array([c - 1 - n_features], np.int64)), const("ax_last", np.array([-1], np.int64)),
                                const("rest_step", np.array([-1], np.int64))], ["rest"]))
    width = n_num + 2 + len(cats_a) + len(cats_b) + 3 + (n_features - c)
    asm = "output" if final == "none" else "assembled"
    nodes.append(node("Concat", ["num_s_out", "sen_i", "hot_a", "hot_b", "flag_b", "rest"], [asm], axis=1))
    ins = [value_info("input", S.FLOAT, ["N", n_features])]
    meta = {"family": "columns", "assembled_width": str(width)}
    if final == "none":
        return model(nodes, ins, [value_info("output", S.FLOAT, ["N", width])], inits, name="columns", metadata=meta)
    if final == "dense":
        inits += [tensor("W", (rng.standard_normal((width, 8)) * 0.3).astype(np.float32)),
                  tensor("B", (rng.standard_normal(8) * 0.1).astype(np.float32))]
        nodes += [node("Gemm", [asm, "W", "B"], ["z"]), node("Relu", ["z"], ["output"])]
        return model(nodes, ins, [value_info("output", S.FLOAT, ["N", 8])], inits, name="columns_dense", metadata=meta)
    trees = [random_complete_tree(rng, depth, width, 1, leaf_scale=0.15) for _ in range(n_trees)]
    a = tree_attrs(trees, "target")
    a.update(n_targets=1, aggregate_function="SUM", post_transform="NONE", base_values=np.array([-0.25], np.float32))
    nodes += [node("TreeEnsembleRegressor", [asm], ["raw"], domain=ML_DOMAIN, **a), node("Sigmoid", ["raw"], ["output"])]
    return model(nodes, ins, [value_info("output", S.FLOAT, ["N", 1])], inits, name="columns_gbdt", metadata=meta)


def tcn(seq: int = 100, in_dim: int = 16, channels=(32, 32), kernel: int = 3, dilations=(1, 2), readout: str = "last",
        layout: int = 0, causal: bool = True, style: str = "pads", residual: bool = True, head: bool = True,
        seed: int = 13, readout_form: str = "default", batch_norm: bool = False, weights=None):
    """Temporal convolutional network (Bai et al.): one residual block per entry of ``channels`` /
    ``dilations``, each ``conv -> Relu -> conv -> Relu``, ``Add`` with the block input (through a k = 1
    Conv where the channel count changes), ``Relu``; ``residual=False`` leaves the plain conv stack.

    ``input`` is [seq, N, in_dim] (``layout`` 0) or [N, seq, in_dim] (1), as the GRU / LSTM builders'; a
    Transpose makes it [N, C, T]. Causal padding is written in one of three ways (``style``): ``pads``
    (the Conv attribute [d (k - 1), 0]), ``chomp`` (symmetric pads, then a Slice dropping the tail: the
    PyTorch export) or ``pad_op`` (a Pad in front of an unpadded Conv); ``causal=False`` pads both sides
    ("same"). ``readout``: ``last`` (Gather axis 2, index -1; ``readout_form="slice"``: Slice + Squeeze),
    ``mean`` / ``max`` (GlobalAveragePool / GlobalMaxPool + Flatten; ``readout_form="reduce"``:
    ReduceMean / ReduceMax over axis 2). Then Gemm -> Sigmoid -> [N, 1]; ``head=False``: the pooled
    [N, C]. ``batch_norm`` puts an inference BatchNormalization behind every block convolution.
    ``weights``: a callable (shape, rng) -> array replacing the random initialisation (integer test
    models)."""
    if len(channels) != len(dilations) or not channels:
        raise ValueError("tcn: one dilation per block")
    if style not in ("pads", "chomp", "pad_op") or readout not in ("last", "mean", "max"):
        raise ValueError("tcn: style pads | chomp | pad_op, readout last | mean | max")
    rng = np.random.default_rng(seed)
    nodes, inits = [], []

    def init(shape, fan):
        if weights is not None:
            return np.asarray(weights(shape, rng), np.float32).reshape(shape)
        s = 1.0 / np.sqrt(fan)
        return rng.uniform(-s, s, shape).astype(np.float32)

    def const(name, arr, scalar=False):
        t = tensor(name, np.asarray(arr))
        if scalar:
            del t.dims[:]
        inits.append(t)
        return name

    def conv(tag, x, cin, cout, k, d, act=True):
        span = d * (k - 1)
        w, b = const(f"{tag}_W", init((cout, cin, k), cin * k)), const(f"{tag}_B", init((cout,), cin * k))
        y = f"{tag}_y"
        if not causal or span == 0:
            nodes.append(node("Conv", [x, w, b], [y], kernel_shape=[k], dilations=[d], pads=[span // 2, span - span // 2]))
        elif style == "pads":
            nodes.append(node("Conv", [x, w, b], [y], kernel_shape=[k], dilations=[d], pads=[span, 0]))
        elif style == "chomp":
            nodes.append(node("Conv", [x, w, b], [f"{tag}_full"], kernel_shape=[k], dilations=[d], pads=[span, span]))
            nodes.append(node("Slice", [f"{tag}_full", const(f"{tag}_s", np.array([0], np.int64)),
                                        const(f"{tag}_e", np.array([-span], np.int64)),
                                        const(f"{tag}_ax", np.array([2], np.int64))], [y]))
        else:
            nodes.append(node("Pad", [x, const(f"{tag}_p", np.array([0, 0, span, 0, 0, 0], np.int64))], [f"{tag}_pad"]))
            nodes.append(node("Conv", [f"{tag}_pad", w, b], [y], kernel_shape=[k], dilations=[d], pads=[0, 0]))
        if batch_norm and act:
            for nm, arr in (("g", rng.uniform(0.5, 1.5, cout)), ("b", rng.uniform(-0.2, 0.2, cout)),
                            ("m", rng.uniform(-0.2, 0.2, cout)), ("v", rng.uniform(0.5, 1.5, cout))):
                const(f"{tag}_bn_{nm}", arr.astype(np.float32))
            nodes.append(node("BatchNormalization", [y] + [f"{tag}_bn_{nm}" for nm in "gbmv"], [f"{tag}_bn"], epsilon=1e-5))
            y = f"{tag}_bn"
        if act:
            nodes.append(node("Relu", [y], [f"{tag}_a"]))
            y = f"{tag}_a"
        return y

    nodes.append(node("Transpose", ["input"], ["x0"], perm=[0, 2, 1] if layout else [1, 2, 0]))
    x, cin = "x0", in_dim
    for bi, (cout, d) in enumerate(zip(channels, dilations)):
        h = conv(f"b{bi}c1", x, cin, cout, kernel, d)
        h = conv(f"b{bi}c2", h, cout, cout, kernel, d)
        if residual:
            skip = x if cin == cout else conv(f"b{bi}ds", x, cin, cout, 1, 1, act=False)
            nodes += [node("Add", [h, skip], [f"b{bi}_sum"]), node("Relu", [f"b{bi}_sum"], [f"b{bi}_out"])]
            h = f"b{bi}_out"
        x, cin = h, cout
    pooled = "pooled" if head else "output"
    if readout == "last" and readout_form == "slice":
        nodes += [node("Slice", [x, const("ro_s", np.array([-1], np.int64)), const("ro_e", np.array([2 ** 31 - 1], np.int64)),
                                 const("ro_ax", np.array([2], np.int64))], ["ro3"]),
                  node("Squeeze", ["ro3", const("ro_sq", np.array([2], np.int64))], [pooled])]
    elif readout == "last":
        nodes.append(node("Gather", [x, const("ro_idx", np.array([-1], np.int64), scalar=True)], [pooled], axis=2))
    elif readout_form == "reduce":
        nodes.append(node("ReduceMean" if readout == "mean" else "ReduceMax", [x], [pooled], axes=[2], keepdims=0))
    else:
        nodes += [node("GlobalAveragePool" if readout == "mean" else "GlobalMaxPool", [x], ["ro3"]),
                  node("Flatten", ["ro3"], [pooled], axis=1)]
    if head:
        const("Wh", init((cin, 1), cin))
        const("Bh", np.zeros(1, np.float32) if weights is None else init((1,), cin))
        nodes += [node("Gemm", ["pooled", "Wh", "Bh"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    x_dims = ["N", seq, in_dim] if layout else [seq, "N", in_dim]
    return model(nodes, [value_info("input", S.FLOAT, x_dims)], [value_info("output", S.FLOAT, ["N", 1 if head else cin])],
                 inits, name="abuse_tcn",
                 metadata={"family": "tcn", "seq": str(seq), "blocks": str(len(channels)), "kernel": str(kernel),
                           "readout": readout, "layout": str(layout)})


BUILDERS = {"qdq_mlp": qdq_mlp, "columns": columns,
            "logistic": logistic, "gbdt": gbdt, "gbdt_v5": gbdt_v5, "stacked": stacked, "ltv_mlp": ltv_mlp, "gru": gru,
            "lstm": lstm, "torch_mlp": torch_mlp, "tabular_resnet": tabular_resnet,
            "sklearn_linear": sklearn_linear, "linear_regressor": linear_regressor,
            "mlp_classifier": mlp_classifier, "wide_deep": wide_deep, "residual_mlp": residual_mlp, "svm": svm}


# sequence models whose graphs use Gather / Slice (BUILDERS lists the families that hold none of the
# column operators, besides ``columns`` itself)
SEQ_BUILDERS = {"tcn": tcn}


def build(kind: str, **kw):
    return (BUILDERS.get(kind) or SEQ_BUILDERS[kind])(**kw)
