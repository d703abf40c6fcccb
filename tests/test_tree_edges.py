"""CPU side of the tree-kernel edge tests: the float64 reference of tests/tree_cases.py against
the C++ executor and the host twins of both device layouts (so trees::compile, to_complete and
to_sparse are checked without a GPU), the dispatch tuple every case must reach, and the proof that
the inputs tell a wrong comparison or a wrong missing bit apart."""
import numpy as np
import pytest

from tests import tree_cases as TC
from tests import tree_models as TM

NAMES = [c.name for c in TC.ALL]


@pytest.fixture(autouse=True)
def _auto_layout(monkeypatch):
    monkeypatch.delenv("IGP_TREE_LAYOUT", raising=False)
    monkeypatch.delenv("IGP_TREE_GROUPS", raising=False)


def _check(case, got, ref, what, budget=1.0):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    if case.exact:
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        r = TC.ratio(got, ref)
        print(f"{case.name} {what}: post {case.post} ratio {r:.4f}")
        assert r <= budget, f"{what}: |err| / (atol + rtol |ref|) = {r}"


@pytest.mark.parametrize("name", NAMES)
def test_executor_and_layout_twins_match_the_float64_walk(name):
    """Exact for the exact cases; else the executor within half of rtol = atol = 1e-5 (the other
    half is the device's), the float32 twins within it."""
    from igaming_platform_amd.native import native
    b = TC.built(name)
    case, step = b.case, b.step
    assert step.layout == case.layout and step.k == case.k and step.n_out == case.n_out
    assert step.n_trees == case.n_trees and step.depth == max(case.depth, 1 if case.layout == "complete" else 0)
    got = native().Executor(b.model).run({"input": np.array(b.X)})["output"]
    _check(case, got, b.ref, "executor", 0.5)
    twin = TC.complete_eval(step, b.X) if case.layout == "complete" else TM.sparse_eval(step, b.X)
    _check(case, twin, b.ref, "layout twin")


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_dispatch_tuple(name):
    b = TC.built(name)
    for g, want in zip(b.case.groups, b.case.expect):
        if b.case.layout == "complete":
            assert TC.complete_dispatch(b.step, b.case.width, g) == want, g
        else:
            assert TC.sparse_dispatch(b.step, g) == want, g


def test_every_listed_branch_is_in_some_asserted_tuple():
    comp = [e for c in TC.COMPLETE for e in c.expect]
    sp = [e for c in TC.SPARSE + [TC.SPARSE_DEPTH0, TC.SPARSE_STRIDE] for e in c.expect]
    kern = {e[0] for e in comp}
    for k in ("K1/scalar", "K2/scalar", "K4/vec4", "K8/vec4", "K16/lpr4/rpt1/tu8+tail", "K32/lpr8/rpt2/tu8+tail",
              "K64/lpr16/rpt4/tu4+tail"):
        assert k in kern, k
    assert {e[1] for e in comp} == {True, False}
    assert {e[2] for e in comp} >= {"scalar", "vec", "vec2", "vec+red"}
    assert {e[3] for e in comp} == {"lds", "lds-overflow", "global"}
    assert {e[4] for e in comp} == {"post_row", "post_elem", "finish_elem", "finish_row"}
    assert {(e[0][:3], e[4]) for e in comp} >= {("K16", "post_elem"), ("K64", "post_row")}   # two-phase epilogues
    assert any(e[5] > 0 and e[0].startswith("K1/") for e in comp) and any(e[5] > 0 and e[0].startswith("K16") for e in comp)
    assert any(e[6] < 4 for e in comp) and any(4 <= e[6] < 16 for e in comp)
    assert {e[0] for e in sp} >= {"KT8>k5", "KT64>k33", "KT1", "KT2"}
    assert {e[1] for e in sp} == {"staged", "global-x"} and {e[2] for e in sp} == {"inline", "finish"}
    assert any(e[3] > 0 for e in sp)
    # item 8 beyond the tuples: what the sparse cases are in the table for
    assert any(e[1] for c in TC.COMPLETE for e in c.expect if e[0][:3] in ("K16", "K32", "K64"))   # two-phase LEQ
    b = TC.built("s_k33_ragged")
    assert {d for tr in b.trees for d in TC.leaf_depths(tr)} == set(range(10)) and b.step.depth == 9
    reached = {len(set(TC.leaf_depths(tr))) for tr in b.trees}
    assert max(reached) >= 5                     # one tree's lanes leave the walk after different visit counts
    assert TC.built("s_depth0").step.depth == 0 and TC.built("s_depth0").step.max_feature == -1
    assert TC.built("s_d14_binary").step.depth == 14 and TC.built("s_k2_avg_probit").step.depth == 13
    assert TC.built("s_stride").step.max_feature + 1 == TC.SPARSE_STRIDE.width < TC.STRIDE_WIDTH
    assert TC.built("s_k5_w260_max").step.max_feature + 1 > 256
    for name, agg, empty in (("s_k5_w260_max", 3, 0), ("s_min81_empty", 2, 1)):
        s = TC.built(name).step
        has = s.leaf_has_np.astype(bool)
        assert s.aggregate == agg and not has[:, 1].any() and has[:, 0].any() and not has[:, 0].all()
        assert max(e[3] for e in TC.BY_NAME[name].expect) == empty and len(TC.BY_NAME[name].groups) == 2
    modes = {m for c in TC.ALL if c.splits for tr in TC.built(c.name).trees for m in tr["mode"]}
    assert modes == set(TC.MODES) | {"LEAF"}
    assert {c.post for c in TC.ALL} == set(TC.POSTS) and {c.agg for c in TC.ALL} == {"SUM", "AVERAGE", "MIN", "MAX"}
    assert {c.kind for c in TC.ALL} == {"reg", "multi", "bin0", "bin1"}


def test_placement_trio_sits_on_both_sides_of_the_lds_limit():
    by = TC.BY_NAME
    a, b = by["place_d10_w16"], by["place_d10_w128"]
    assert [t["feature"].tolist() for t in TC.built(a.name).trees] == [t["feature"].tolist() for t in TC.built(b.name).trees]
    assert TC.built(a.name).step.n_trees * ((1 << 10) - 1) == 9207 > TC.STAGE_NODES
    on, past = by["place_96k_w121"], by["place_96k_w122"]
    assert sum(TC.complete_bytes(1, 8, 33, on.width)) == TC.LDS_LIMIT
    assert sum(TC.complete_bytes(1, 8, 33, past.width)) == TC.LDS_LIMIT + 256
    assert np.array_equal(TC.built(on.name).step.nodes_np, TC.built(past.name).step.nodes_np)


@pytest.mark.parametrize("name", [c.name for c in TC.ALL if c.layout == "complete" and c.shape == "ragged"])
def test_ragged_cases_pad_the_complete_layout(name):
    """A single-leaf tree and a depth-1 leaf are in every ragged ensemble: to_complete's dummy
    nodes (+inf, LEQ, missing-true) are in the node table the kernel reads."""
    b = TC.built(name)
    assert (b.trees[1]["feature"] < 0).all() and len(b.trees[1]["feature"]) == 1
    assert b.trees[2]["feature"][b.trees[2]["left"][0]] < 0
    nodes = b.step.nodes_np.reshape(b.step.n_trees, -1, 2)
    assert np.isinf(nodes[1, :, 0]).all() and np.isinf(nodes[..., 0]).sum() > nodes.shape[1]


@pytest.mark.parametrize("name", [c.name for c in TC.ALL if c.splits])
def test_inputs_discriminate(name):
    """A quarter of the X entries on a threshold, 2 % NaN; LEQ -> LT with GTE -> GT changes at
    least a quarter of the rows, the inverted missing bit one row in twenty."""
    b = TC.built(name)
    on, nan = TC.input_stats(b.trees, b.X)
    assert on >= 0.25 and 0.01 <= nan <= 0.04, (on, nan)
    X = b.X
    assert np.isinf(X).any() and (X == 0).any() and np.signbit(X[X == 0]).any()
    read = set(TC.column_thresholds(b.trees))
    assert np.isnan(X[:, [c for c in range(X.shape[1]) if c not in read]]).all()
    modes = {m for tr in b.trees for m in tr["mode"]}
    strict = TC.case_ref(b.case, b.trees, X, strict=True)
    changed = float(np.mean(np.any(strict != b.ref, axis=1)))
    assert modes & {"BRANCH_LEQ", "BRANCH_GTE"} and changed >= 0.25, changed
    flipped = TC.case_ref(b.case, b.trees, X, flip_missing=True)
    changed = float(np.mean(np.any(flipped != b.ref, axis=1)))
    assert changed >= 0.05, changed


def test_depth0_is_the_only_case_without_a_comparison():
    for c in TC.ALL:
        has = any((tr["feature"] >= 0).any() for tr in TC.built(c.name).trees)
        assert has == c.splits == (c.name != "s_depth0")
    assert TC.built("s_depth0").step.depth == 0


@pytest.mark.parametrize("name", [c.name for c in TC.ALL if c.layout == "sparse"])
def test_sparse_cases_pass_the_upload_check(name):
    """validate_sparse used to refuse s_depth0: with no inner node its largest feature id was
    taken as 0, above the max_feature = -1 of an ensemble that reads no feature."""
    from igaming_platform_amd.models.plan import validate_sparse
    validate_sparse(TC.built(name).step)


def test_eq_and_neq_nodes_meet_zero_and_nan():
    """BRANCH_EQ / BRANCH_NEQ thresholds at 0 with +-0.0 in X; NaN under NEQ goes to the true side
    whatever the missing bit says, under every other mode only with it."""
    tr = dict(feature=np.array([0, -1, -1]), threshold=np.zeros(3, np.float32), left=np.array([1, 0, 0]),
              right=np.array([2, 0, 0]), mode=["BRANCH_EQ", "LEAF", "LEAF"], missing_true=np.array([0, 0, 0]),
              leaf_values=np.array([[0], [1], [2]], np.float32))
    X = np.array([[0.0], [-0.0], [np.nan], [1.0]], np.float32)
    assert TC.ref_walk([tr], X, 1)[:, 0].tolist() == [1, 1, 2, 2]
    tr["mode"][0] = "BRANCH_NEQ"
    assert TC.ref_walk([tr], X, 1)[:, 0].tolist() == [2, 2, 1, 1]
    tr["mode"][0], tr["missing_true"] = "BRANCH_GTE", np.array([1, 0, 0])
    assert TC.ref_walk([tr], X, 1)[:, 0].tolist() == [1, 1, 1, 1]
    assert TC.ref_walk([tr], X, 1, flip_missing=True)[:, 0].tolist() == [1, 1, 2, 1]
    assert TC.ref_walk([tr], X, 1, strict=True)[:, 0].tolist() == [2, 2, 1, 1]
    assert any(t == 0 and m in ("BRANCH_EQ", "BRANCH_NEQ") for c in TC.COMPLETE for trr in TC.built(c.name).trees
               for t, m in zip(trr["threshold"], trr["mode"]))


def test_tree_groups_leaves_trailing_groups_empty():
    from types import SimpleNamespace
    from igaming_platform_amd.engine.runner import tree_groups
    for T, groups, empty in ((161, 20, 2), (129, 16, 1), (81, 10, 1), (128, 16, 0)):
        g = tree_groups(SimpleNamespace(n_trees=T), 64)
        assert g == groups and sum(nt <= 0 for nt in TC.group_sizes(T, g)) == empty, (T, g)


def test_stacked_parts_are_the_builders_draws():
    """tree_cases.stacked_parts reproduces builders.stacked: the executor on the built model is
    within half the budget of ref_walk -> ref64 on the parts."""
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    N = native()
    om = N.OnnxModel.from_bytes(builders.stacked(n_trees=129, depth=4, k=32, hidden=100).SerializeToString())
    X = np.random.default_rng(6).uniform(0, 1, (64, 128)).astype(np.float32)
    got = np.asarray(N.Executor(om).run({"input": X})["output"])[:, 0]
    trees, head = TC.stacked_parts(129, hidden=100)
    r = TC.ratio(got, TC.stacked_ref(trees, head, X))
    print(f"stacked executor ratio {r:.4f}")
    assert r <= 0.5
