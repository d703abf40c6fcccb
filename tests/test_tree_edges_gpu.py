"""K2 (trees.hip: tree_kernel<K, LEQ>, the finish kernels, tree_head_kernel) and K2b
(trees_sparse.hip) on every dispatch path, against the float64 walk of tests/tree_cases.py.

X sits in a NaN-poisoned buffer (columns no node reads, rows past n_rows), the partial slab of
every grouped launch is poisoned before the launch: NaN for SUM / AVERAGE, so that a group that stores
nothing makes the finisher's sum NaN; -3e38 for MIN and +3e38 for MAX, finite values that win the
finisher's fminf / fmaxf (which drop a NaN), so an empty group has to store its +-inf. Outputs sit in a buffer pre-filled with -7 whose rows
past n_rows must stay bit-identical. SUM / MIN / MAX cases without a post transform must equal the
reference; the others use rtol = atol = 1e-5 against float64. Which kernel instance, loader, node
placement and finisher a case reaches is asserted in tests/test_tree_edges.py."""
from functools import lru_cache

import numpy as np
import pytest

from tests import dense_cases as D
from tests import tree_cases as TC

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


@lru_cache(maxsize=None)
def _on_device(name):
    """(built case, its TreeStep uploaded)."""
    from igaming_platform_amd.models.plan import Plan, to_device
    b = TC.built(name)
    to_device(Plan("t", b.case.width, [b.step], b.step.n_out, 0, {}, "input", "output"), "cuda")
    return b


def _compare(case, Y, ref, rows, what):
    got = Y[:rows].double().numpy()
    print(f"{case.name} {what} rows {rows}: ratio {TC.ratio(got, ref[:rows]):.4f}")
    if case.exact:
        np.testing.assert_array_equal(got, ref[:rows], err_msg=what)
    else:
        np.testing.assert_allclose(got, ref[:rows], rtol=TC.RTOL, atol=TC.ATOL, err_msg=what)
    assert D.untouched(Y, rows, Y.shape[1]), f"{what}: wrote past n_rows"


def _poison(aggregate=0):
    """What a slab holds before a grouped launch: the value a group that stores nothing leaves
    behind must spoil the result. fminf / fmaxf return their non-NaN operand, so MIN (2) / MAX (3)
    get a finite value that wins instead (an infinity would be read as "no tree wrote this target")."""
    return {2: -3e38, 3: 3e38}.get(aggregate, float("nan"))


def _nan_slab(groups, rows, k, aggregate=0):
    torch = _t()
    return torch.full((max(groups, 1) * rows * k,), _poison(aggregate), dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------ K2
@pytest.mark.parametrize("rows", TC.ROWS)
@pytest.mark.parametrize("name", [c.name for c in TC.COMPLETE])
def test_complete_kernel_every_dispatch_path(name, rows):
    """One group (the in-kernel epilogues) and every grouped launch of the case (finish kernels,
    ragged and empty groups) at 1, 63, 65 and 130 rows."""
    torch, K = _t(), _K()
    b = _on_device(name)
    case, step = b.case, b.step
    Xd = D.poisoned(rows + 9, rows, case.width, case.width, torch.float32, np.array(b.X)).cuda()
    for g in case.groups:
        Y = D.sentinel_out(rows + 9, step.n_out, torch.float32).cuda()
        K.tree_ensemble(step, Xd, Y, rows, partial=_nan_slab(g, rows, step.k) if g > 1 else None, groups=g)
        _compare(case, Y.cpu(), b.ref, rows, f"groups {g}")


# ------------------------------------------------------------------------------ K2b
def _sparse_run(b, rows, width):
    torch, K = _t(), _K()
    case, step = b.case, b.step
    Xd = D.poisoned(rows + 9, rows, width, case.width, torch.float32, np.array(b.X)).cuda()
    for g in case.groups:
        Y = D.sentinel_out(rows + 9, step.n_out, torch.float32).cuda()
        K.tree_sparse(step, Xd, Y, rows, partial=_nan_slab(g, rows, step.k, step.aggregate) if g > 1 else None,
                      groups=g)
        _compare(case, Y.cpu(), b.ref, rows, f"groups {g}")


@pytest.mark.parametrize("rows", TC.ROWS)
@pytest.mark.parametrize("name", [c.name for c in TC.SPARSE + [TC.SPARSE_DEPTH0]])
def test_sparse_kernel_every_dispatch_path(name, rows):
    """KT instances wider than k, the X tile staged and read from global memory, MIN / MAX with
    targets no leaf writes and an empty group, depth 0 and depth 14, lanes that reach their leaves
    after 0 to 9 edges."""
    _sparse_run(_on_device(name), rows, TC.BY_NAME[name].width)


@pytest.mark.parametrize("rows", TC.ROWS)
def test_sparse_kernel_row_stride_wider_than_the_staged_tile(rows):
    """x_stride = 24 while the kernel stages max_feature + 1 = 12 columns; columns 12.. are NaN."""
    b = _on_device(TC.SPARSE_STRIDE.name)
    assert b.step.max_feature + 1 == TC.SPARSE_STRIDE.width < TC.STRIDE_WIDTH
    _sparse_run(b, rows, TC.STRIDE_WIDTH)


# ------------------------------------------------------------------------------ tree -> head
def _head_step(W1, b1, act1, w2, b2, act2):
    from igaming_platform_amd.models.plan import HeadStep, Plan, to_device
    hs = HeadStep(n1=W1.shape[0], k=W1.shape[1], act1=act1, act2=act2, w1_np=W1, b1_np=b1, w2_np=w2, b2=b2)
    to_device(Plan("t", W1.shape[1], [hs], 1, 0, {}, "input", "output"), "cuda", "fp32")
    return hs


def test_tree_head_live_rows_inside_a_tile_and_seven_groups():
    """tree_head_kernel called directly: 50 mixed-mode K = 32 trees in 7 groups (8, ..., 8, 2), 130
    rows of which m_ptr says 70 are live (tile 1 ends inside, tile 2 has none), a 40-column X, a
    NaN slab; the tickets are back at zero and rows 70.. of Y untouched."""
    torch, K = _t(), _K()
    from igaming_platform_amd.models.plan import Plan, compile_onnx, to_device
    from igaming_platform_amd.native import native
    case = TC.Case("head_k32", "complete", "reg", 32, 50, 4, 40, (7,), (), modes="four", n_base=32, seed=30)
    trees = TC.make_trees(case)
    for tr in trees:    # multiples of 2^-15 below 1 / 8: still exact sums, O(1) head pre-activations
        tr["leaf_values"] = tr["leaf_values"] / np.float32(32)
    (step,) = compile_onnx(native().OnnxModel.from_bytes(TC.make_model(case, trees).SerializeToString())).steps
    to_device(Plan("t", 40, [step], 32, 0, {}, "input", "output"), "cuda")
    assert TC.complete_dispatch(step, 40, 7)[:4] == ("K32/lpr8/rpt2/tu8+tail", False, "vec", "lds")
    rows, live, N1 = 130, 70, 100
    _, W1, b1, w2, b2 = D.head_operands(32, N1)
    hs = _head_step(W1, b1, "tanh", w2, b2, "sigmoid")
    assert K.tree_head_ok(step, hs, 7)
    X = TC.make_X(trees, rows, 40, case.seed)
    Xd = D.poisoned(rows + 9, rows, 40, 40, torch.float32, X).cuda()
    Y = D.sentinel_out(rows + 9, 2, torch.float32).cuda()
    slab = _nan_slab(7, rows, 32)
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    m = torch.tensor([live], dtype=torch.int32, device="cuda")
    K.tree_head(step, hs, Xd, Y, rows, slab, 7, cnt, m_ptr=m)
    Y = Y.cpu()
    emb = TC.ref_walk(trees, X[:live], 32, base=TC.base_values(case))
    ref = D.ref64(emb, head=(W1, b1, "tanh", w2, b2, "sigmoid"))
    np.testing.assert_allclose(Y[:live, 0].double().numpy(), ref[:, 0], rtol=TC.RTOL, atol=TC.ATOL)
    assert D.untouched(Y, live, 1)
    assert int(cnt.abs().sum()) == 0
    part = slab.cpu().view(7, rows, 32)    # every group stored its rows: exact sums of exact leaves
    np.testing.assert_array_equal(part.double().sum(0).numpy() + TC.base_values(case).astype(np.float64),
                                  TC.ref_walk(trees, X, 32, base=TC.base_values(case)))


# ------------------------------------------------------------------------------ the auto rule
def _device_model(b, width, bucket=64):
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import Plan
    plan = Plan("gbdt", width, [b.step], b.step.n_out, 0, {}, "input", "output")
    return DeviceModel(plan, "cuda", [bucket])


@pytest.mark.parametrize("name,groups,empty", [("k1_t161_binary_logistic", 20, 2), ("s_min81_empty", 10, 1)])
def test_device_model_auto_groups_leave_empty_groups(name, groups, empty):
    """DeviceModel at a 64-row bucket with IGP_TREE_GROUPS unset: runner.tree_groups picks 20
    groups for 161 trees (two empty) and 10 for 81 (one empty), one run per layout; the model's slab
    is poisoned before the run (NaN; -3e38 for the MIN model)."""
    torch = _t()
    b = _on_device(name)
    dm = _device_model(b, b.case.width)
    assert dm.tree_groups[64] == groups
    assert sum(nt <= 0 for nt in TC.group_sizes(b.step.n_trees, groups)) == empty
    dm.tree_partial.fill_(_poison(b.step.aggregate))
    Xd = D.poisoned(64, 63, b.case.width, b.case.width, torch.float32, np.array(b.X)).cuda()
    out = dm.run(Xd, 64)
    torch.cuda.synchronize()
    got = out[:63].cpu().double().numpy()
    if b.case.exact:
        np.testing.assert_array_equal(got, b.ref[:63])
    else:
        np.testing.assert_allclose(got, b.ref[:63], rtol=TC.RTOL, atol=TC.ATOL)
