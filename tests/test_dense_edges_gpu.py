"""K3 (gemm.hip, mlp_fused.hip, join.hip) at odd widths, strides wider than the live width and
every dispatch path, against the float64 references of tests/dense_cases.py.

Inputs sit in NaN-poisoned buffers (every element outside the live [:M, :K] block is NaN) and
outputs in buffers pre-filled with -7 that must stay bit-identical outside [:M, :N]: a kernel that
reads past K / M or writes past N / M fails the comparison, no fault needed. Which kernel branch a
case reaches is the comment next to it (here and in dense_cases.py).

Tolerances are the suite's own: fp32 dense rtol 1e-5 / atol 2e-5 and fp32 head 1e-5 against
float64; bf16 dense 2e-3, head 3e-3, chain 2e-3 against the bf16-convention reference; the split
chain 1e-4 (max error over max reference) against pure float64; device models 1e-5 (fp32) and
3e-2 (bf16) against the C++ executor."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from tests import dense_cases as D

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16"]
TOL_DENSE = {"fp32": dict(rtol=1e-5, atol=2e-5), "bf16": dict(rtol=2e-3, atol=2e-3)}
TOL_HEAD = {"fp32": dict(rtol=1e-5, atol=1e-5), "bf16": dict(rtol=3e-3, atol=3e-3)}
TOL_CHAIN = dict(rtol=2e-3, atol=2e-3)
TOL_MODEL = {"fp32": 1e-5, "bf16": 3e-2}


def _t():
    import torch
    return torch


def _K():
    from igaming_platform_amd.ops import kernels as K
    return K


def _pad(precision):
    from igaming_platform_amd.models.plan import _bf16_padded, _f32_padded
    return _f32_padded if precision == "fp32" else _bf16_padded


def _ldx(K, mode):
    """scalar: rows 4 / 2 bytes off every 16-byte boundary (the per-element loaders); vector:
    16-byte-aligned rows wider than K (the float4 / uint4 loaders)."""
    return K + 3 if mode == "scalar" else -(-K // 8) * 8 + 8


def _i32(v):
    torch = _t()
    return torch.tensor([v], dtype=torch.int32, device="cuda")


@lru_cache(maxsize=None)
def _dense_case(case):
    X, W, b = D.dense_operands(case)
    act = case[3]
    return X, W, b, {False: D.ref64(X, [(W, b, act)]), True: D.ref64(X, [(W, b, act)], bf16=True)}


# ------------------------------------------------------------------------------ dense / GEMV
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", D.DENSE_CASES, ids=D.dense_id)
def test_dense_tails_strides_and_bounds(case, precision):
    """gemm_kernel<64,64> / <128,128> (bf16 W), gemm_f32_kernel (f32 W) and gemv_kernel (N = 1):
    K, N and M tails, the scalar (ldx = K + 3) and the vector (ldx % 8 == 0, > K) A loaders for
    f32 and bf16 X, ldy = N + 5, live rows through m_ptr with 9 poisoned rows behind them."""
    torch, K = _t(), _K()
    M, N, Kd, act, xbf = case
    X, W, b, refs = _dense_case(case)
    ref = torch.from_numpy(refs[precision == "bf16"]).float()
    Wd, bd, m = _pad(precision)(W).cuda(), torch.from_numpy(b).cuda(), _i32(M)
    if precision == "bf16" and N > 1:
        assert (M + 9 >= 4096 and N >= 128) == (M == 4097)   # launch_gemm's 128x128 tile choice
    for mode in ("scalar", "vector"):
        Xd = D.poisoned(M + 9, M, _ldx(Kd, mode), Kd, torch.bfloat16 if xbf else torch.float32, X).cuda()
        Y = D.sentinel_out(M + 9, N + 5, torch.float32).cuda()
        K.dense(Xd, Wd, bd, Y, M + 9, N, Kd, act=act, m_ptr=m)
        Y = Y.cpu()
        torch.testing.assert_close(Y[:M, :N], ref, msg=lambda s: f"ldx {mode}: {s}", **TOL_DENSE[precision])
        assert D.untouched(Y, M, N), f"ldx {mode}: wrote outside [:M, :N]"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ldy", [100, 103])
def test_dense_bf16_output_stride(ldy, precision):
    """y_bf16 stores with ldy == N and ldy > N (2-byte elements: a row 206 bytes long). The f32
    result is rounded once to bf16: half a bf16 ulp (<= 2^-8 |y|) on top of the family's tolerance."""
    torch, K = _t(), _K()
    M, N, Kd, act, xbf = D.DENSE_YBF16
    X, W, b, refs = _dense_case(D.DENSE_YBF16)
    ref = refs[precision == "bf16"]
    Wd, bd, m = _pad(precision)(W).cuda(), torch.from_numpy(b).cuda(), _i32(M)
    for mode in ("scalar", "vector"):
        Xd = D.poisoned(M + 9, M, _ldx(Kd, mode), Kd, torch.bfloat16, X).cuda()
        Y = D.sentinel_out(M + 9, ldy, torch.bfloat16).cuda()
        K.dense(Xd, Wd, bd, Y, M + 9, N, Kd, act=act, m_ptr=m)
        Y = Y.cpu()
        got = Y[:M, :N].float().numpy().astype(np.float64)
        tol = TOL_DENSE[precision]
        assert np.all(np.abs(got - ref) <= tol["atol"] + (tol["rtol"] + 2.0 ** -8) * np.abs(ref))
        assert D.untouched(Y, M, N)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dense_live_row_count(precision):
    """m_ptr = 0 writes nothing; m_ptr inside a tile writes exactly that many rows; m_ptr > M is
    clamped to M."""
    torch, K = _t(), _K()
    case = D.DENSE_CASES[1]
    M, N, Kd, act, _ = case
    X, W, b, refs = _dense_case(case)
    ref = torch.from_numpy(refs[precision == "bf16"]).float()
    Wd, bd = _pad(precision)(W).cuda(), torch.from_numpy(b).cuda()
    Xd = D.poisoned(M + 9, M, Kd + 3, Kd, torch.float32, X).cuda()
    for live, m_arg, want in ((0, M + 9, 0), (37, M + 9, 37), (1000, M, M)):
        Y = D.sentinel_out(M + 9, N + 5, torch.float32).cuda()
        K.dense(Xd, Wd, bd, Y, m_arg, N, Kd, act=act, m_ptr=_i32(live))
        Y = Y.cpu()
        torch.testing.assert_close(Y[:want, :N], ref[:want], **TOL_DENSE[precision])
        assert D.untouched(Y, want, N), (live, m_arg)


# ------------------------------------------------------------------------------ join
def _join_case(op, na, nb, da, db, dy):
    torch, K = _t(), _K()
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}
    rng = np.random.default_rng(4000 + na + 3 * nb)
    # multiples of 2^-8 below 8: every sum is exact in f32, so "rounded once" has one meaning
    A = np.round(rng.standard_normal((70, na)) * 256) / 256
    B = np.round(rng.standard_normal((70, nb)) * 256) / 256
    Ah = D.bf16r(A) if da == "bf16" else A      # the values the operand tensors hold
    Bh = D.bf16r(B) if db == "bf16" else B
    want = D.ref_join(op, Ah, Bh)
    want = D.bf16r(want) if dy == "bf16" else want.astype(np.float32).astype(np.float64)
    width = want.shape[1]
    Ad = D.poisoned(79, 70, na + 3, na, dt[da], A).cuda()
    Bd = D.poisoned(79, 70, nb + 3, nb, dt[db], B).cuda()
    Y = D.sentinel_out(79, width + 3, dt[dy]).cuda()
    K.join(op, Ad, Bd, Y, 79, na, nb, m_ptr=_i32(70))   # 70 * width ends inside a 256-thread block
    Y = Y.cpu()
    np.testing.assert_array_equal(Y[:70, :width].float().numpy().astype(np.float64), want)
    assert D.untouched(Y, 70, width)


@pytest.mark.parametrize("dy", ["f32", "bf16"])
@pytest.mark.parametrize("db", ["f32", "bf16"])
@pytest.mark.parametrize("da", ["f32", "bf16"])
@pytest.mark.parametrize("op,na,nb", [("add", 100, 100), ("concat", 100, 33)])
def test_join_mixed_dtypes_and_strides(op, na, nb, da, db, dy):
    """join_kernel: every f32 / bf16 combination of A, B and Y, lda / ldb / ldy 3 wider than the
    live widths, 70 live rows of 79 through m_ptr; exact against float64 rounded once."""
    _join_case(op, na, nb, da, db, dy)


@pytest.mark.parametrize("na,nb", [(1, 1), (64, 64)])
def test_join_concat_widths(na, nb):
    _join_case("concat", na, nb, "f32", "f32", "f32")
    _join_case("concat", na, nb, "bf16", "f32", "bf16")


# ------------------------------------------------------------------------------ fused head
def _head_step(precision, Kd, N1, act1, act2, W1, b1, w2, b2):
    from igaming_platform_amd.models.plan import HeadStep, Plan, to_device
    hs = HeadStep(n1=N1, k=Kd, act1=act1, act2=act2, w1_np=W1, b1_np=b1, w2_np=w2, b2=b2)
    to_device(Plan("t", Kd, [hs], 1, 0, {}, "input", "output"), "cuda", precision)
    return hs


@pytest.mark.parametrize("case", D.HEAD_CASES, ids=D.head_id)
def test_head_dispatch_paths_and_tails(case):
    """mlp_head_f32_fast_kernel (KP 32 / 64; the W1 loop past 8 chunks per thread, the n >= 256
    b1 / w2 loop, N1 tails), mlp_head_f32_kernel (W1 in LDS at k_pad 96 / 128, W1 from global) and
    mlp_head_kernel (bf16; W1 in LDS / from global, f32 and bf16 X), ldx = K + 3."""
    torch, K = _t(), _K()
    precision, Kd, N1, act1, act2, xbf, kern, w_lds = case
    X, W1, b1, w2, b2 = D.head_operands(Kd, N1, xbf=xbf)
    hs = _head_step(precision, Kd, N1, act1, act2, W1, b1, w2, b2)
    k_pad = hs.w1.shape[1]
    assert k_pad == -(-Kd // (32 if precision == "fp32" else 64)) * (32 if precision == "fp32" else 64)
    assert D.head_dispatch(precision, k_pad, N1) == (kern, w_lds)   # the case still reaches its kernel
    if kern == "fast64" and N1 == 320:
        assert -(-N1 // 64) * 64 * k_pad // 4 > 2048                  # W1 chunks beyond 8 per thread
    Xd = D.poisoned(79, D.HEAD_M, Kd + 3, Kd, torch.bfloat16 if xbf else torch.float32, X).cuda()
    Y = D.sentinel_out(79, 2, torch.float32).cuda()
    K.mlp_head(hs, Xd, Y, 79, m_ptr=_i32(D.HEAD_M))
    Y = Y.cpu()
    ref = D.ref64(X, head=(W1, b1, act1, w2, b2, act2), bf16=precision == "bf16")
    torch.testing.assert_close(Y[:D.HEAD_M, 0], torch.from_numpy(ref[:, 0]).float(), **TOL_HEAD[precision])
    assert D.untouched(Y, D.HEAD_M, 1)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("with_base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("average", [0, 1], ids=["sum", "avg"])
@pytest.mark.parametrize("groups,k", [
    (1, 32), (8, 32),    # head_a_f32: the straight-line path (groups <= 8, clamped group index)
    (9, 32), (25, 32),   # the groups > 8 loop (DeviceModel: 64-row bucket, >= 136 trees)
    (3, 12),             # K % 4 == 0: chunk 0 vector, chunk 8..11 scalar (kc + 8 > K)
    (3, 10),             # K % 4 != 0: scalar
    (12, 6),             # K < 8 and groups > 8: scalar
])
def test_head_tree_partial_staging(groups, k, average, with_base, precision):
    """The head reduces [groups, M, k] tree partials while staging: (sum_g slab[g]) / n_trees + base,
    with and without p_average / pbase. The slab is the input: no trees needed."""
    torch, K = _t(), _K()
    M, N1 = D.HEAD_M, 64
    _, W1, b1, w2, b2 = D.head_operands(k, N1)
    rng = np.random.default_rng(5000 + 10 * groups + k)
    slab = (0.3 * rng.standard_normal((groups, M, k))).astype(np.float32)
    base = (0.2 * rng.standard_normal(k)).astype(np.float32) if with_base else None
    hs = _head_step(precision, k, N1, "relu", "sigmoid", W1, b1, w2, b2)
    ts = SimpleNamespace(k=k, post=0, binary_class=-1, average=average, n_trees=37,
                         base=None if base is None else torch.from_numpy(base).cuda())
    Y = D.sentinel_out(79, 2, torch.float32).cuda()
    K.mlp_head(hs, None, Y, M, tree_partial=(torch.from_numpy(slab).cuda(), groups, ts))
    Y = Y.cpu()
    xin = slab.astype(np.float64).sum(0)
    if average:
        xin = xin / 37
    if base is not None:
        xin = xin + base
    ref = D.ref64(xin, head=(W1, b1, "relu", w2, b2, "sigmoid"), bf16=precision == "bf16")
    torch.testing.assert_close(Y[:M, 0], torch.from_numpy(ref[:, 0]).float(), **TOL_HEAD[precision])
    assert D.untouched(Y, M, 1)


def _stacked(n_trees, hidden, poison=False):
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    torch = _t()
    N = native()
    om = N.OnnxModel.from_bytes(builders.stacked(n_trees=n_trees, depth=4, k=32, hidden=hidden).SerializeToString())
    plan = to_device(compile_onnx(om), "cuda")
    assert [s.kind for s in plan.steps] == ["tree", "head"]
    dm = DeviceModel(plan, "cuda", [64])
    if poison:   # a group that stores nothing leaves NaN for the reduction
        dm.tree_partial.fill_(float("nan"))
    X = np.random.default_rng(6).uniform(0, 1, (64, 128)).astype(np.float32)
    ref = np.asarray(N.Executor(om).run({"input": X})["output"])[:, 0]
    out = dm.run(torch.from_numpy(X).cuda(), 64)
    torch.cuda.synchronize()
    return dm, plan, out[:, 0].cpu().numpy(), ref


@pytest.mark.parametrize("hidden", [100, 512])
def test_tree_head_one_launch_at_16_groups(hidden, monkeypatch):
    """trees.hip tree_head_kernel at the tree_head_ok limit (16 groups: 128 trees in a 64-row
    bucket) with an N1 tail (100) and the widest head (512), against the C++ executor."""
    monkeypatch.setenv("IGP_TREE_HEAD", "1")
    monkeypatch.delenv("IGP_TREE_GROUPS", raising=False)
    dm, plan, got, ref = _stacked(128, hidden)
    assert dm.tree_groups[64] == 16 and _K().tree_head_ok(plan.steps[0], plan.steps[1], 16)
    assert int(dm.tile_cnt.abs().sum()) == 0
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=0)
    assert np.ptp(ref) > 1e-3


def test_tree_head_one_launch_with_an_empty_last_group(monkeypatch):
    """129 trees in a 64-row bucket: 16 groups of 9, group 14 holds 3 trees and group 15 none; its
    blocks still store zeros into the (NaN-poisoned) slab and take their tickets. Against the
    float64 walk of the trees pushed through the float64 head (tests/tree_cases.py)."""
    from tests import tree_cases as TC
    monkeypatch.setenv("IGP_TREE_HEAD", "1")
    monkeypatch.delenv("IGP_TREE_GROUPS", raising=False)
    dm, plan, got, ref = _stacked(129, 100, poison=True)
    assert dm.tree_groups[64] == 16 and _K().tree_head_ok(plan.steps[0], plan.steps[1], 16)
    assert TC.group_sizes(129, 16)[-2:] == [3, -6]
    assert int(dm.tile_cnt.abs().sum()) == 0
    trees, head = TC.stacked_parts(129, hidden=100)
    X = np.random.default_rng(6).uniform(0, 1, (64, 128)).astype(np.float32)
    np.testing.assert_allclose(got, TC.stacked_ref(trees, head, X), **TOL_HEAD["fp32"])
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=0)
    assert not bool(_t().isnan(dm.tree_partial[:16 * 64 * 32]).any())


def test_tree_head_routing_past_16_groups(monkeypatch):
    """200 trees in a 64-row bucket: 25 groups, tree_head_ok refuses, the plan runs
    tree_ensemble(no_finish) then mlp_head reducing 25 group partials (head_a_f32's groups > 8 loop)."""
    monkeypatch.delenv("IGP_TREE_GROUPS", raising=False)
    dm, plan, got, ref = _stacked(200, 100)
    assert dm.tree_groups[64] == 25 and not _K().tree_head_ok(plan.steps[0], plan.steps[1], 25)
    np.testing.assert_allclose(got, ref, atol=1e-5, rtol=0)
    assert np.ptp(ref) > 1e-3


# ------------------------------------------------------------------------------ MLP chain
def _chain_run(name, rows, split, X, lay, head, monkeypatch, live=D.CHAIN_LIVE):
    torch, K = _t(), _K()
    monkeypatch.setenv("IGP_MLP_ROWS", rows)
    monkeypatch.setenv("IGP_MLP_SPLIT_ROWS", rows)
    pk = K.MlpChainPack(D.chain_steps(lay, head), torch.device("cuda", 0), split=split)
    assert pk.waves() == D.CHAIN_CASES[name][3]
    in_live = X.shape[1]
    Xd = D.poisoned(D.CHAIN_N, live, in_live + 3, in_live, torch.float32, X).cuda()
    ml = torch.full((D.CHAIN_N,), D.SENTINEL, device="cuda")
    K.mlp_chain(pk, D.CHAIN_N, X=Xd, ml=ml, m_ptr=_i32(live))
    torch.cuda.synchronize()
    return ml.cpu()


def _chain_check(ml, X, lay, head, split, live=D.CHAIN_LIVE):
    torch = _t()
    assert torch.all(ml[live:] == D.SENTINEL)
    got = ml[:live].numpy().astype(np.float64)
    if split:   # f32-faithful: against pure float64
        ref = D.ref64(X, lay, head)[:live, 0]
        assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-4
    else:
        ref = D.ref64(X, lay, head, bf16=True)[:live, 0]
        np.testing.assert_allclose(got, ref, **TOL_CHAIN)


@pytest.mark.parametrize("name,rows,split", [
    ("30-64-64", "16", False),      # mlp_chain_kernel<16, 4, false>
    ("30-64-64", "32", False),      # <32, 4, false>
    ("30-64-64", "64", False),      # <64, 4, false>
    ("1-192-64", "32", False),      # <32, 4, false>, in_live = 1, NT = 3 column tiles per wave
    ("1-192-64", "32", True),       # <32, 4, true>
    ("65-128-256", "32", False),    # <32, 8, false>, in_live one past a 64-column k-tile
    ("65-128-256", "64", False),    # <64, 8, false>
    ("65-128-256", "32", True),     # <32, 8, true>
    ("65-128-256", "64", True),     # <64, 8, true, NBUF = 1>
    ("512-512-128", "32", True),    # <32, 8, true> at the widest layer (16 k-steps)
    ("512-512-128", "64", True),    # <64, 8, true, NBUF = 1>
])
def test_chain_every_instantiation(name, rows, split, monkeypatch):
    """Every mlp_chain_kernel instantiation of launch_mlp_chain, with sigmoid and tanh hidden
    layers (mc_act), in_live tails of 1, 30 and 65, ldx = in_live + 3 and 66 live rows of 70."""
    X, lay, head = D.chain_operands(name)
    ml = _chain_run(name, rows, split, X, lay, head, monkeypatch)
    _chain_check(ml, X, lay, head, split)


# ------------------------------------------------------------------------------ saturation
SAT_ROWS = range(8, 24)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_dense_saturates_finite(act, precision):
    torch, K = _t(), _K()
    M, N, Kd = 65, 100, 100
    X, W, b = D.dense_operands((M, N, Kd, act, False))
    X = D.saturating_rows(X, W, b, SAT_ROWS)
    ref = D.ref64(X, [(W, b, act)], bf16=precision == "bf16")
    assert np.abs(ref[8:24] - np.round(ref[8:24])).max() < 1e-20   # the reference there is 0, 1 or -1
    Y = torch.zeros(M, N, device="cuda")
    K.dense(torch.from_numpy(X).cuda(), _pad(precision)(W).cuda(), torch.from_numpy(b).cuda(), Y, M, N, Kd, act=act)
    Y = Y.cpu()
    assert torch.isfinite(Y).all()
    torch.testing.assert_close(Y, torch.from_numpy(ref).float(), **TOL_DENSE[precision])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act1,act2", [("sigmoid", "tanh"), ("tanh", "sigmoid")])
def test_head_saturates_finite(act1, act2, precision):
    torch, K = _t(), _K()
    X, W1, b1, w2, b2 = D.head_operands(100, 64)
    X = D.saturating_rows(X, W1, b1, SAT_ROWS)
    hs = _head_step(precision, 100, 64, act1, act2, W1, b1, w2, b2)
    Y = torch.zeros(D.HEAD_M, 1, device="cuda")
    K.mlp_head(hs, torch.from_numpy(X).cuda(), Y, D.HEAD_M)
    Y = Y.cpu()
    ref = D.ref64(X, head=(W1, b1, act1, w2, b2, act2), bf16=precision == "bf16")
    assert torch.isfinite(Y).all()
    torch.testing.assert_close(Y, torch.from_numpy(ref).float(), **TOL_HEAD[precision])


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
@pytest.mark.parametrize("acts,act2", [(("sigmoid", "tanh"), "sigmoid"), (("tanh", "sigmoid"), "tanh")])
def test_chain_saturates_finite(acts, act2, split, monkeypatch):
    X, lay, head = D.chain_operands("30-64-64", acts, act2)
    X = D.saturating_rows(X, lay[0][0], lay[0][1], SAT_ROWS)
    ml = _chain_run("30-64-64", "32", split, X, lay, head, monkeypatch)
    assert np.isfinite(ml[:D.CHAIN_LIVE].numpy()).all()
    _chain_check(ml, X, lay, head, split)


# ------------------------------------------------------------------------------ row isolation
def _isolated(run, X):
    """Row 17 of X zero / NaN / +Inf: every other row's output is bit-identical (rows are
    independent in all of these kernels, so no tolerance)."""
    torch = _t()
    outs = []
    for v in (0.0, float("nan"), float("inf")):
        Xv = np.array(X, np.float32)
        Xv[17] = v
        outs.append(run(Xv))
    keep = torch.arange(outs[0].shape[0]) != 17
    for o in outs[1:]:
        assert torch.equal(outs[0][keep].view(torch.int32), o[keep].view(torch.int32))
    assert torch.isfinite(outs[0][keep]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dense_rows_isolated_from_nonfinite_row(precision):
    torch, K = _t(), _K()
    M, N, Kd = 65, 100, 100
    X, W, b = D.dense_operands((M, N, Kd, "tanh", False))
    Wd, bd = _pad(precision)(W).cuda(), torch.from_numpy(b).cuda()

    def run(Xv):
        Y = torch.zeros(M, N, device="cuda")
        K.dense(torch.from_numpy(Xv).cuda(), Wd, bd, Y, M, N, Kd, act="tanh")
        return Y.cpu()
    _isolated(run, X)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_head_rows_isolated_from_nonfinite_row(precision):
    torch, K = _t(), _K()
    X, W1, b1, w2, b2 = D.head_operands(100, 64)
    hs = _head_step(precision, 100, 64, "tanh", "sigmoid", W1, b1, w2, b2)

    def run(Xv):
        Y = torch.zeros(D.HEAD_M, 1, device="cuda")
        K.mlp_head(hs, torch.from_numpy(Xv).cuda(), Y, D.HEAD_M)
        return Y.cpu()
    _isolated(run, X)


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "split"])
def test_chain_rows_isolated_from_nonfinite_row(split, monkeypatch):
    X, lay, head = D.chain_operands("30-64-64")
    _isolated(lambda Xv: _chain_run("30-64-64", "32", split, Xv, lay, head, monkeypatch, live=D.CHAIN_N), X)


# ------------------------------------------------------------------------------ NaN parity with the CPU twin
def _device_and_executor(model_bytes, X, precision):
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    torch = _t()
    N = native()
    om = N.OnnxModel.from_bytes(model_bytes)
    plan = to_device(compile_onnx(om), "cuda", precision)
    dm = DeviceModel(plan, "cuda", [64])
    Xd = torch.zeros((64, X.shape[1]), dtype=torch.float32, device="cuda")
    Xd[:X.shape[0]] = torch.from_numpy(X).cuda()
    out = dm.run(Xd, 64)
    torch.cuda.synchronize()
    ref = np.asarray(N.Executor(om).run({"input": X})["output"]).reshape(X.shape[0], -1)
    return plan, out[:X.shape[0]].float().cpu().numpy(), ref


def _nonfinite_X(K):
    X = np.random.default_rng(7).standard_normal((37, K)).astype(np.float32)
    X[3] = np.nan            # a whole NaN row
    X[5, 2] = np.inf         # one +Inf / -Inf / NaN element
    X[7, 2] = -np.inf
    X[9, K - 1] = np.nan
    return X


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act", ["none", "relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("N", [33, 1], ids=["gemm", "gemv"])
def test_dense_nan_rows_match_the_executor(N, act, precision):
    """The CPU executor answers the same traffic on failover: the same rows are NaN on both
    (relu is x > 0 ? x : 0 on both, so NaN -> 0), the finite ones agree."""
    rng = np.random.default_rng(8)
    W = (rng.standard_normal((N, 30)) / np.sqrt(30)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    X = _nonfinite_X(30)
    plan, got, ref = _device_and_executor(D.onnx_mlp([(W, b, act)]), X, precision)
    assert [s.kind for s in plan.steps] == ["dense"]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], ref[fin], atol=TOL_MODEL[precision], rtol=TOL_MODEL[precision])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("act1", ["none", "relu", "sigmoid", "tanh"])
@pytest.mark.parametrize("K,N1", [(30, 100), (100, 100)], ids=["fast", "generic"])
def test_head_nan_rows_match_the_executor(K, N1, act1, precision):
    """... through the fused head with an N1 tail. The head's padded hidden columns (zero W1 rows,
    N1..n1p) turn an Inf input into 0 x Inf = NaN in the accumulator; the three mlp_head kernels
    used to add act1(NaN) * 0 = NaN to the row sum there (read from their code while this test was
    written), which makes a row with one Inf feature NaN on the device and finite (sigmoid / tanh
    saturate) in the executor. The kernels now skip those columns."""
    _, W1, b1, w2, b2 = D.head_operands(K, N1, M=37)
    X = _nonfinite_X(K)
    head = (W1, b1, act1, w2, b2, "sigmoid")
    plan, got, ref = _device_and_executor(D.onnx_mlp(D.head_layers(head)), X, precision)
    assert [s.kind for s in plan.steps] == ["head"]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    np.testing.assert_allclose(got[fin], ref[fin], atol=TOL_MODEL[precision], rtol=TOL_MODEL[precision])


# ------------------------------------------------------------------------------ odd-shaped models end to end
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind,kw,kinds", D.MODEL_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(D.MODEL_CASES)])
def test_odd_shaped_model_matches_executor(kind, kw, kinds, precision):
    """An sklearn-default-shaped MLP (30 features, 100 hidden units) through compile_onnx ->
    to_device -> DeviceModel: the fast f32 head at an N1 tail; dense -> head and dense -> dense ->
    head with activation rows of ldx = 100 (bf16 plans: 200-byte rows, the per-element loader of
    gemm_kernel's x_bf16 branch and of the bf16 head)."""
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    torch = _t()
    N = native()
    om = N.OnnxModel.from_bytes(builders.build(kind, **kw).SerializeToString())
    plan = to_device(compile_onnx(om), "cuda", precision=precision)
    assert [s.kind for s in plan.steps] == kinds
    dm = DeviceModel(plan, "cuda", [64])
    assert [t.shape[1] for t in dm.step_out] == [100] * (len(kinds) - 1) + [1]
    rng = np.random.default_rng(11)
    for rows in (1, 37, 64):
        X = rng.standard_normal((rows, 30)).astype(np.float32)
        ref = np.asarray(N.Executor(om).run({"input": X})["output"]).reshape(rows, -1)[:, plan.executor_col]
        Xd = torch.zeros((64, 30), dtype=torch.float32, device="cuda")
        Xd[:rows] = torch.from_numpy(X).cuda()
        out = dm.run(Xd, 64)
        torch.cuda.synchronize()
        got = out[:rows, plan.ml_col].float().cpu().numpy()
        np.testing.assert_allclose(got, ref, atol=TOL_MODEL[precision], rtol=TOL_MODEL[precision])
