"""Cases, inputs and a float64 reference for the opset-5 ``TreeEnsemble`` operator and its
set-membership splits (tests/test_tree_member.py on the CPU, tests/test_tree_member_gpu.py on the
device).

The reference (:func:`walk64`) walks the per-tree dicts the model was written from, one row and
one node at a time: a member node goes to its true branch when ``float32(x) == float32(m)`` for
some member m (so -0.0 matches 0.0 and NaN matches nothing), or when x is NaN and the node tracks
missing values to the true side. Nothing in it passed through trees::compile, the set encoder or
a bisection. Leaves are non-zero multiples of 2^-10 below 4 and each leaf writes one target, as the
operator defines: SUM / MIN / MAX results without a post transform are exact in float32 in any
order and must EQUAL the reference; the other cases use tree_cases' rtol = atol = 1e-5.

The named sets (:data:`SETS`) are the smallest shapes at which the device's two set encodings can
go wrong; ``kind`` is the encoding each must take (CAP = 256): bitset for integers in [0, CAP),
sorted value list for everything else."""
import os
from contextlib import contextmanager
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace
from typing import Tuple

import numpy as np

from tests import tree_cases as TC

CAP = 256
BITSET, LIST = 0, 1
_spread = lambda n: sorted(int(v) for v in (np.arange(n) * 7) % CAP)   # n distinct integers in [0, CAP)
_rng100 = np.random.default_rng(77)

# name -> (members, encoding)
SETS = {
    "bits_0": ([], BITSET),
    "bits_1": ([5], BITSET),
    "bits_2": ([3, 200], BITSET),
    "bits_31": (_spread(31), BITSET),
    "bits_32": (_spread(32), BITSET),
    "bits_33": (_spread(33), BITSET),
    "bits_cap": (list(range(CAP)), BITSET),
    "edge_31": ([31], BITSET),
    "edge_32": ([32], BITSET),
    "edge_cap_m1": ([CAP - 1], BITSET),
    "edge_cap": ([CAP], LIST),
    "edge_cap_m1_cap": ([CAP - 1, CAP], LIST),
    "list_neg3": ([-3.0], LIST),
    "list_halves": ([0.5, 2.5], LIST),
    "list_1e30": ([1e30], LIST),
    "list_inf": ([np.inf], LIST),
    "list_negzero": ([-0.0], BITSET),   # -0.0 == 0.0: the integer 0
    "list_100": (sorted(float(v) for v in ((_rng100.choice(8000, 100, replace=False) - 4000) * 2 + 1) / 16.0), LIST),
}
SET_NAMES = list(SETS)


def members32(name):
    return np.asarray(SETS[name][0], np.float32)


def probes(name, full):
    """The probe values of one set. ``full``: around every member (the CPU tier); otherwise around
    at most 20 representative members (first, last, next to a 32-bit word edge), so that a set's
    probes fit the 130 rows of the device tier."""
    m = [float(v) for v in members32(name)]
    out = [np.nan, 0.0, -0.0, -1.0, float(CAP), float(CAP - 1), 1e30, np.inf, -np.inf, 2.5]
    if SETS[name][1] == BITSET:
        reps = m if full else sorted(set(m[:2] + m[-2:] + [v for v in m if int(v) % 32 in (0, 31)]))[:20]
        for v in reps:
            out += [v, v - 1, v + 1, v + 0.5, -v]
    else:
        picks = sorted(set([m[0], m[len(m) // 2], m[-1]])) if not full else m
        for v in picks:
            f = np.float32(v)
            out += [float(f), float(np.nextafter(f, np.float32(-np.inf))), float(np.nextafter(f, np.float32(np.inf)))]
        lo, hi = np.float32(m[0]), np.float32(m[-1])
        out += [float(lo) - 1.0 if np.isfinite(lo) else -3e38, float(hi) + 1.0 if np.isfinite(hi) else 3e38]
    with np.errstate(over="ignore"):
        return np.asarray(out, np.float64).astype(np.float32)


# ------------------------------------------------------------------------------ tree builders
def _leaf_rows(rng, n, k):
    """[n, k] float32: one non-zero multiple of 2^-10 below 4 per row, and the column it sits in."""
    tgt = rng.integers(0, k, n)
    w = rng.integers(1, 4096, n) * rng.choice([-1, 1], n) / 1024.0
    lv = np.zeros((n, k), np.float32)
    lv[np.arange(n), tgt] = w
    return lv, tgt


def one_target(rng, tr, k, scale=None):
    """Rewrite the leaves of a tree_cases tree so that each writes one target (the operator's
    leaves are (target, weight) pairs). ``scale``: inexact normal weights instead of dyadic ones."""
    leaf = np.flatnonzero(np.asarray(tr["feature"]) < 0)
    lv, tgt = _leaf_rows(rng, len(leaf), k)
    if scale is not None:
        lv = (lv * np.float32(scale / 2.0) * np.float32(1.0009765)).astype(np.float32)
    tr["leaf_values"] = np.zeros((len(tr["feature"]), k), np.float32)
    tr["leaf_values"][leaf] = lv
    tr["leaf_target"] = np.full(len(tr["feature"]), -1, np.int64)
    tr["leaf_target"][leaf] = tgt
    return tr


def node_depths(tr):
    d = np.zeros(len(tr["feature"]), np.int64)
    stack = [0]
    while stack:
        i = stack.pop()
        if tr["feature"][i] >= 0:
            for c in (int(tr["left"][i]), int(tr["right"][i])):
                d[c] = d[i] + 1
                stack.append(c)
    return d


def memberize(rng, tr, where, share, depth):
    """Turn interior nodes into BRANCH_MEMBER nodes on sets drawn from :data:`SETS`. ``where``:
    root, last (the nodes at depth - 1), or any (a ``share`` of all interior nodes)."""
    n = len(tr["feature"])
    tr["mode"] = list(tr["mode"])
    tr["members"] = [None] * n
    tr["set_name"] = [None] * n
    inner = np.flatnonzero(np.asarray(tr["feature"]) >= 0)
    if where == "root":
        pick = inner[inner == 0]
    elif where == "last":
        pick = inner[node_depths(tr)[inner] == depth - 1]
    else:
        pick = inner[rng.uniform(0, 1, len(inner)) < share]
    for i in pick:
        name = SET_NAMES[int(rng.integers(0, len(SET_NAMES)))]
        tr["mode"][i] = "BRANCH_MEMBER"
        tr["members"][i] = members32(name)
        tr["set_name"][i] = name
        tr["threshold"][i] = 0.0
    return tr


def chain_tree(rng, depth, used, k):
    """A spine of ``depth`` interior nodes, every second one a member node; the side that goes on
    alternates, the other child is a leaf. Depth-first order, the root first."""
    feat, thr, mode, miss, left, right = [], [], [], [], [], []

    def add(f=-1, t=0.0, m="LEAF", ms=0):
        for a, v in zip((feat, thr, mode, miss, left, right), (f, np.float32(t), m, ms, 0, 0)):
            a.append(v)
        return len(feat) - 1
    cur = add()
    for d in range(depth):
        f, t, m, ms = TC._inner(rng, used, TC.MODES, TC.GRID)
        feat[cur], thr[cur], mode[cur], miss[cur] = f, t, m, ms
        if d % 2 == 0:   # true side is the leaf
            left[cur] = add()
            right[cur] = nxt = add()
        else:
            left[cur] = nxt = add()
            right[cur] = add()
        cur = nxt
    n = len(feat)
    tr = dict(feature=np.array(feat, np.int64), threshold=np.array(thr, np.float32), left=np.array(left, np.int64),
              right=np.array(right, np.int64), mode=mode, missing_true=np.array(miss, np.int64),
              leaf_values=np.zeros((n, k), np.float32))
    tr["members"], tr["set_name"] = [None] * n, [None] * n
    spine = [i for i in range(n) if feat[i] >= 0]
    for j, i in enumerate(spine):
        if j % 2 == 1 or j == 0 or j == len(spine) - 1:
            name = SET_NAMES[int(rng.integers(0, len(SET_NAMES)))]
            tr["mode"][i], tr["members"][i], tr["set_name"][i], tr["threshold"][i] = "BRANCH_MEMBER", members32(name), name, 0.0
    return tr


@dataclass(frozen=True)
class MCase:
    name: str
    layout: str
    k: int
    n_trees: int
    depth: int
    width: int
    groups: Tuple[int, ...]
    where: str = "any"
    share: float = 0.4
    shape: str = "full"
    modes: str = "six"
    agg: str = "SUM"
    post: str = "NONE"
    p_leaf: float = 0.3
    n_used: int = 10
    seed: int = 0
    chain: bool = False        # tree 0 a depth-``depth`` chain, tree 1 a single leaf
    nodes: str = "lds"         # where launch_kl puts the node table at one group

    @property
    def exact(self):
        return self.post == "NONE" and self.agg in ("SUM", "MIN", "MAX")


def make_trees(case):
    rng = np.random.default_rng(12000 + case.seed)
    used = TC.used_columns(SimpleNamespace(cols_width=0, width=case.width, n_used=case.n_used), rng)
    trees = []
    for t in range(case.n_trees):
        if case.chain and t == 0:
            tr = chain_tree(rng, case.depth, used, case.k)
        elif case.chain and t == 1:
            tr = memberize(rng, TC.make_tree(rng, 0, used, case.k, TC.MODES, force="leaf"), "any", 0, 0)
        else:
            d = min(case.depth, 5) if case.chain else case.depth
            tr = TC.make_tree(rng, d, used, case.k, TC.MODE_SETS[case.modes], case.shape, case.p_leaf)
            memberize(rng, tr, case.where, case.share, d)
        trees.append(one_target(rng, tr, case.k, None if case.exact or case.post == "SOFTMAX_ZERO" else 1.0))
    return trees


V5_AGG = {"AVERAGE": 0, "SUM": 1, "MIN": 2, "MAX": 3}
V5_POST = {"NONE": 0, "SOFTMAX": 1, "LOGISTIC": 2, "SOFTMAX_ZERO": 3, "PROBIT": 4}


def model_v5(trees, k, width, agg="SUM", post="NONE", name="member", trailing_nan=True):
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import ML_DOMAIN, model, node, tree_attrs_v5, value_info
    nd = node("TreeEnsemble", ["input"], ["output"], domain=ML_DOMAIN, n_targets=k, aggregate_function=V5_AGG[agg],
              post_transform=V5_POST[post], **tree_attrs_v5(trees, trailing_nan=trailing_nan))
    return model([nd], [value_info("input", S.FLOAT, ["N", width])], [value_info("output", S.FLOAT, ["N", k])],
                 name=name, ml_opset=5)


# ------------------------------------------------------------------------------ inputs
def probe_pool(trees):
    """column -> the probe values of every set a member node tests that column against."""
    cols = {}
    for tr in trees:
        for i, name in enumerate(tr.get("set_name", [])):
            if name is not None:
                cols.setdefault(int(tr["feature"][i]), []).append(probes(name, False))
    return {c: np.unique(np.concatenate(v)) for c, v in cols.items()}   # unique keeps one NaN


def make_X(trees, n_rows, width, seed):
    """tree_cases.make_X (thresholds, NaN, infinities, both zeros; unread columns NaN), then 60 % of
    the entries of every column a member node reads are drawn from that column's probe values."""
    X = TC.make_X(trees, n_rows, width, seed)
    rng = np.random.default_rng(12500 + seed)
    for c, pool in probe_pool(trees).items():
        take = rng.uniform(0, 1, n_rows) < 0.6
        X[:, c] = np.where(take, pool[rng.integers(0, len(pool), n_rows)], X[:, c])
    return X


# ------------------------------------------------------------------------------ the reference
def _true(mode, x, thr, members, miss):
    x = np.float32(x)
    if mode == "BRANCH_MEMBER":
        c = bool(np.any(np.asarray(members, np.float32) == x))
    else:
        t = np.float32(thr)
        c = bool({"BRANCH_LEQ": x <= t, "BRANCH_LT": x < t, "BRANCH_GTE": x >= t, "BRANCH_GT": x > t,
                  "BRANCH_EQ": x == t, "BRANCH_NEQ": x != t}[mode])
    return c or (bool(miss) and bool(np.isnan(x)))


def walk64(trees, X, k, agg="SUM", post="NONE"):
    """float64 [rows, k]: every leaf writes its one target (``leaf_target``); MIN / MAX leave a
    target no visited leaf writes at 0."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    init = {"SUM": 0.0, "AVERAGE": 0.0, "MIN": np.inf, "MAX": -np.inf}[agg]
    acc = np.full((n, k), init, np.float64)
    for tr in trees:
        feat, members = tr["feature"], tr.get("members") or [None] * len(tr["feature"])
        for r in range(n):
            i = 0
            while feat[i] >= 0:
                go = _true(tr["mode"][i], X[r, feat[i]], tr["threshold"][i], members[i], tr["missing_true"][i])
                i = int(tr["left"][i] if go else tr["right"][i])
            t = int(tr["leaf_target"][i])
            w = float(tr["leaf_values"][i][t])
            acc[r, t] = acc[r, t] + w if agg in ("SUM", "AVERAGE") else min(acc[r, t], w) if agg == "MIN" else max(acc[r, t], w)
    if agg in ("MIN", "MAX"):
        acc[np.isinf(acc)] = 0.0
    if agg == "AVERAGE":
        acc /= len(trees)
    return TC.post64(post, acc)


# ------------------------------------------------------------------------------ the probe model
PROBE_K = 64


def probe_trees():
    """Per named set two depth-1 trees (missing tracks false / true) on the set's own column,
    writing 1 (member) or 0.25 to their own target; then the set-order tree: a non-member root
    whose two children are member nodes on ONE column with different sets, stored right child first,
    so the order of the member nodes in nodes_modes is not the order a traversal meets them."""
    trees = []
    for s, name in enumerate(SET_NAMES):
        for miss in (0, 1):
            t = 2 * s + miss
            lv = np.zeros((3, PROBE_K), np.float32)
            lv[1, t], lv[2, t] = 1.0, 0.25
            trees.append(dict(feature=np.array([s, -1, -1], np.int64), threshold=np.zeros(3, np.float32),
                              left=np.array([1, 0, 0], np.int64), right=np.array([2, 0, 0], np.int64),
                              mode=["BRANCH_MEMBER", "LEAF", "LEAF"], missing_true=np.array([miss, 0, 0], np.int64),
                              leaf_values=lv, leaf_target=np.array([-1, t, t], np.int64),
                              members=[members32(name), None, None], set_name=[name, None, None]))
    a, b, t0 = len(SET_NAMES), len(SET_NAMES) + 1, 2 * len(SET_NAMES)
    lv = np.zeros((7, PROBE_K), np.float32)
    tgt = np.full(7, -1, np.int64)
    for j, leaf in enumerate((3, 4, 5, 6)):
        lv[leaf, t0 + j], tgt[leaf] = 0.5 + j, t0 + j
    trees.append(dict(feature=np.array([a, b, b, -1, -1, -1, -1], np.int64),
                      threshold=np.array([0.5, 0, 0, 0, 0, 0, 0], np.float32),
                      left=np.array([2, 3, 5, 0, 0, 0, 0], np.int64), right=np.array([1, 4, 6, 0, 0, 0, 0], np.int64),
                      mode=["BRANCH_LEQ", "BRANCH_MEMBER", "BRANCH_MEMBER", "LEAF", "LEAF", "LEAF", "LEAF"],
                      missing_true=np.zeros(7, np.int64), leaf_values=lv, leaf_target=tgt,
                      members=[None, np.array([2, 40], np.float32), np.array([1, 300], np.float32), None, None, None, None],
                      set_name=[None] * 7))
    return trees


PROBE_WIDTH = 20   # 18 set columns, the set-order tree's two


def probe_X(full):
    cols = [probes(name, full) for name in SET_NAMES]
    cols += [np.array([0.0, 1.0, np.nan, 0.5], np.float32), np.array([1, 2, 40, 300, 3, np.nan], np.float32)]
    n = max(len(c) for c in cols) if full else TC.N_ROWS
    assert all(len(c) <= n for c in cols)
    X = np.stack([np.resize(c, n) for c in cols], 1).astype(np.float32)
    # the set-order columns: every pairing within the first rows
    X[:24, PROBE_WIDTH - 2] = np.repeat(cols[-2], 6)
    X[:24, PROBE_WIDTH - 1] = np.tile(cols[-1], 4)
    return X


# ------------------------------------------------------------------------------ the case table
M = MCase
COMPLETE = [
    # depth 1: every node a member node at the root; K = 1; 5 groups of 5 (the last holds 4)
    M("c_d1_k1_root", "complete", 1, 24, 1, 16, (1, 5), where="root", n_used=16, seed=1),
    # depth 3, K = 32 (leaf-vector two-phase path), member nodes at the last level; 4 groups of 6 (last 3)
    M("c_d3_k32_last", "complete", 32, 21, 3, 40, (1, 4), where="last", seed=2),
    # depth 5, ragged, member nodes among all six comparison modes; K = 1; 3 groups of 5 (last 3)
    M("c_d5_k1_mixed", "complete", 1, 13, 5, 30, (1, 3), shape="ragged", seed=3),
    # ... at K = 32; 5 groups of 8 (last 5)
    M("c_d5_k32_mixed", "complete", 32, 37, 5, 40, (1, 5), shape="ragged", seed=4),
    # row-wise finish (tree_finish_kernel): SOFTMAX over 4 targets, AVERAGE
    M("c_d3_k4_softmax", "complete", 4, 11, 3, 16, (1, 3), agg="AVERAGE", post="SOFTMAX", seed=5),
    # 9 trees of depth 10 behind a 128-column X: the node table stays in global memory at one
    # group, two groups stage theirs in LDS
    M("c_d10_global", "complete", 1, 9, 10, 128, (1, 2), share=0.3, n_used=16, seed=6, nodes="global"),
]
SPARSE = [
    # a depth-14 chain with member nodes along it, a single-leaf tree, ragged member trees; SUM
    M("s_chain14_sum", "sparse", 3, 9, 14, 30, (1, 3), shape="ragged", chain=True, seed=10),
    # X read from global memory (a node reads column 259), MAX
    M("s_w260_max", "sparse", 5, 11, 4, 260, (1, 3), shape="ragged", agg="MAX", seed=11),
    # MIN, staged X
    M("s_min", "sparse", 3, 10, 4, 16, (1, 3), shape="ragged", agg="MIN", seed=12),
    # AVERAGE + LOGISTIC, a chain again
    M("s_avg_logistic", "sparse", 2, 7, 13, 24, (1, 3), shape="ragged", agg="AVERAGE", post="LOGISTIC", chain=True,
      seed=13),
]
ALL = COMPLETE + SPARSE
BY_NAME = {c.name: c for c in ALL}


@contextmanager
def forced_layout(layout):
    old = os.environ.get("IGP_TREE_LAYOUT")
    os.environ["IGP_TREE_LAYOUT"] = layout
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("IGP_TREE_LAYOUT", None)
        else:
            os.environ["IGP_TREE_LAYOUT"] = old


def compile_step(model_proto, layout):
    """(OnnxModel, the single TreeStep) of a one-operator model on the forced layout."""
    from igaming_platform_amd.models.plan import compile_onnx
    from igaming_platform_amd.native import native
    om = native().OnnxModel.from_bytes(model_proto.SerializeToString())
    with forced_layout(layout):
        (step,) = compile_onnx(om).steps
    assert step.layout == layout
    return om, step


@lru_cache(maxsize=None)
def built(name):
    """The case's trees, model, TreeStep on the case's layout, X [N_ROWS, width], float64 reference."""
    case = BY_NAME[name]
    trees = make_trees(case)
    om, step = compile_step(model_v5(trees, case.k, case.width, case.agg, case.post, case.name), case.layout)
    X = make_X(trees, TC.N_ROWS, case.width, case.seed)
    ref = walk64(trees, X, case.k, case.agg, case.post)
    ref.setflags(write=False)
    X.setflags(write=False)
    return SimpleNamespace(case=case, trees=trees, model=om, step=step, X=X, ref=ref)


@lru_cache(maxsize=None)
def built_probe(layout, full=False):
    trees = probe_trees()
    om, step = compile_step(model_v5(trees, PROBE_K, PROBE_WIDTH, name="probe"), layout)
    X = probe_X(full)
    ref = walk64(trees, X, PROBE_K)
    ref.setflags(write=False)
    X.setflags(write=False)
    return SimpleNamespace(trees=trees, model=om, step=step, X=X, ref=ref)


# ------------------------------------------------------------------------------ stacked (cfg3 shape)
def stacked_member_parts(n_trees, share=0.35, seed=3):
    """tree_cases.stacked_parts' trees and head, with a ``share`` of member nodes on sets of small
    feature-scaled values and one target per leaf (the operator's leaves are (target, weight) pairs)."""
    trees, head = TC.stacked_parts(n_trees, hidden=100, seed=seed)
    rng = np.random.default_rng(13000 + seed)
    for tr in trees:
        tr["feature"] = np.asarray(tr["feature"]).copy()
        memberize(rng, tr, "any", share, 4)
        leaf = np.flatnonzero(tr["feature"] < 0)
        tgt = rng.integers(0, 32, len(leaf))
        tr["leaf_values"] = np.zeros((len(tr["feature"]), 32), np.float32)
        lv = (rng.standard_normal(len(leaf)) * 0.4).astype(np.float32)
        lv[lv == 0] = np.float32(0.1)
        tr["leaf_values"][leaf, tgt] = lv
        tr["leaf_target"] = np.full(len(tr["feature"]), -1, np.int64)
        tr["leaf_target"][leaf] = tgt
    return trees, head


def stacked_member_model(trees, head):
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import ML_DOMAIN, model, node, tensor, tree_attrs_v5, value_info
    W1, b1, _, w2, b2, _ = head
    nodes = [node("TreeEnsemble", ["input"], ["emb"], domain=ML_DOMAIN, n_targets=32, aggregate_function=V5_AGG["SUM"],
                  post_transform=0, **tree_attrs_v5(trees)),
             node("Gemm", ["emb", "W1", "B1"], ["h1"]), node("Relu", ["h1"], ["a1"]),
             node("Gemm", ["a1", "W2", "B2"], ["logit"]), node("Sigmoid", ["logit"], ["output"])]
    inits = [tensor("W1", np.ascontiguousarray(W1.T)), tensor("B1", b1), tensor("W2", np.ascontiguousarray(w2[:, None])),
             tensor("B2", np.array([b2], np.float32))]
    return model(nodes, [value_info("input", S.FLOAT, ["N", 128])], [value_info("output", S.FLOAT, ["N", 1])], inits,
                 name="stacked_member", ml_opset=5)


def stacked_member_ref(trees, head, X):
    from tests.dense_cases import ref64
    return ref64(walk64(trees, X, 32), head=head)[:, 0]


# ------------------------------------------------------------------------------ scikit-learn
CATS = {1: [0.5 * c - 3.0 for c in range(40)]}    # column 1: the raw value of each ordinal code


def hgb_data(n=2000, seed=5):
    """(X as scikit-learn sees it: ordinal codes; X as the exported model sees it: column 1 holds
    the raw values; y). Columns 0 / 1 categorical (12 / 40 categories), 2..5 on a grid of eighths;
    3 % NaN in every column."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, 6), np.float64)
    X[:, 0] = rng.integers(0, 12, n)
    X[:, 1] = rng.integers(0, 40, n)
    X[:, 2:] = rng.integers(0, 64, (n, 4)) / 8.0
    y = (np.isin(X[:, 0], [1, 4, 5, 9]) * 2.0 + np.isin(X[:, 1] % 7, [0, 3]) * 1.5 + (X[:, 2] > 3.1) - 0.3 * X[:, 3]
         + rng.standard_normal(n) * 0.1)
    X[rng.uniform(0, 1, X.shape) < 0.03] = np.nan
    raw = X.copy()
    ok = ~np.isnan(X[:, 1])
    raw[ok, 1] = np.asarray(CATS[1])[X[ok, 1].astype(int)]
    return X, raw.astype(np.float32), y


@lru_cache(maxsize=None)
def hgb_model(kind):
    from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor
    from igaming_platform_amd.onnx import convert
    X, raw, y = hgb_data()
    kw = dict(max_iter=20, max_depth=5, categorical_features=[0, 1], random_state=0)
    if kind == "clf":
        est = HistGradientBoostingClassifier(**kw).fit(X, y > np.median(y))
        ref = est.predict_proba(X)[:, 1]
    else:
        est = HistGradientBoostingRegressor(**kw).fit(X, y)
        ref = est.predict(X)
    n_cat = sum(int(p[0].nodes["is_categorical"][~p[0].nodes["is_leaf"].astype(bool)].sum()) for p in est._predictors)
    return convert.hist_gradient_boosting(est, 6, categories=CATS), raw, ref, n_cat, est


# ------------------------------------------------------------------------------ engine
NOW = 1_760_000_000


def engine_config():
    from igaming_platform_amd.config import Config
    cfg = Config()
    cfg.gpu.buckets = [64, 256]
    cfg.gpu.max_batch = 256
    return cfg


def engine_model():
    """An opset-5 fraud model on the engine's feature width whose member nodes test the small
    integer columns (transaction counts, unique devices / addresses) against sets of 0 .. 7."""
    from igaming_platform_amd.onnx import builders
    return builders.build("gbdt_v5", n_trees=20, depth=4, n_features=engine_config().features.width, member_share=0.6,
                          n_categorical=8, categories=8).SerializeToString()


def engine_txs(n, rng, n_acc=40):
    types = ["deposit", "withdraw", "bet", "win", "bonus"]
    return [dict(account_id=f"acc-{int(a)}", amount=int(rng.choice([500, 5000, 150000, 2_000_000])),
                 transaction_type=types[int(rng.integers(0, 5))], device_id=f"dev-{int(a)}-{int(rng.integers(0, 5))}",
                 ip_address=f"10.1.{int(a)}.{int(rng.integers(0, 7))}", fingerprint=f"fp-{int(a)}")
            for a in rng.integers(0, n_acc, n)]
