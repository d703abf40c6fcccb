"""The decision kernels on the device against the golden, exactly (tables and references:
tests/decision_cases.py; their self-checks and the host twins: tests/test_decision_edges.py).

K5 ``ensemble_row`` with a model output on its six hosts - ensemble_kernel over every table, with
ml_col / ml_stride, dead rows, host_out and the routed host rows; the three mlp_head kernels, the
tree finish kernel and tree_head_kernel with a model that puts the table's ml values on the rows -
K10 as exact counter deltas, K9 ``ltv_row`` in ltv_kernel and in the epilogue of every
mlp_chain_kernel instance, and ltv_assemble_kernel against float64."""
from functools import lru_cache

import numpy as np
import pytest

from tests import decision_cases as DC
from tests import dense_cases as D
from tests import tree_cases as TC

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 9   # rows allocated behind n_rows: nothing may touch them


def _t():
    import torch
    return torch


def _K():
    from igaming_platform_amd.ops import kernels as K
    return K


def _res_out(rows):
    torch = _t()
    return torch.full((rows, 2), DC.RES_SENTINEL, dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class Batch:
    """Device operands of one K5 launch over ``tab`` rows (n_rows >= len(tab): zero FeatRecs behind)."""

    def __init__(self, name, tab, n_rows, n_live, ml_col=0, ml_stride=1):
        torch = _t()
        tab = {k: v[:n_rows] for k, v in tab.items()}
        self.sc, self.tab, self.n_rows, self.n_live = DC.k5_scoring(name), tab, n_rows, n_live
        self.hdr = torch.from_numpy(DC.k5_hdr(n_live)).cuda()
        self.cfg = torch.from_numpy(DC.k5_cfg_bytes(name, ml_col, ml_stride)).cuda()
        self.feat = torch.from_numpy(DC.k5_feat(tab, n_rows).view(np.int32).copy()).cuda()
        self.X = torch.full((n_rows, 1), float("nan"), device="cuda")   # the heuristic's input: not read
        self.flags = np.zeros(n_rows, np.int32)
        self.flags[:len(tab["flags"])] = tab["flags"]
        self.out = _res_out(n_rows + PAD)
        self.metrics = torch.zeros(128, dtype=torch.int64, device="cuda")

    def golden(self, ml):
        """Records of the launch for the float32 model outputs ``ml`` [n_rows]."""
        n = self.n_rows
        rule, reasons = np.zeros(n, np.int32), np.zeros(n, np.int32)
        rule[:len(self.tab["rule"])], reasons[:len(self.tab["rule"])] = self.tab["rule"], self.tab["reasons"]
        return DC.k5_golden(self.sc, rule, reasons, self.flags, ml, self.n_live)

    def args(self, ml, metrics=True, out=None, **kw):
        return _K().ensemble_args(self.hdr, self.cfg, self.feat, self.X, ml, self.out if out is None else out,
                                  self.n_rows, self.metrics if metrics else None, **kw)

    def check(self, out, want, what):
        got = _u32(out)
        bad = np.nonzero((got[:self.n_rows] != want).any(1))[0]
        assert not len(bad), f"{what}: {len(bad)} rows differ, first {bad[:5]}: {got[bad[:3]]} != {want[bad[:3]]}"
        assert (got[self.n_rows:] == DC.RES_SENTINEL).all(), f"{what}: wrote past n_rows"


def _ml_buffer(ml, n_rows, col, stride):
    """[n_rows + PAD, stride] float32 with ``ml`` in column ``col`` and NaN everywhere else."""
    torch = _t()
    buf = np.full((n_rows + PAD, stride), np.nan, F32)
    buf[:len(ml), col] = ml
    return torch.from_numpy(buf).cuda()


# ------------------------------------------------------------------------------ K5 standalone + K10
@pytest.mark.parametrize("name", list(DC.K5_CONFIGS))
def test_ensemble_kernel_whole_table_and_metrics(name):
    """Every row of the config's table, with and without metrics; the counters grow by exactly
    the golden's counts, also on a second launch onto non-zero counters."""
    torch, K = _t(), _K()
    tab = DC.k5_table(name)
    n = len(tab["rule"])
    b = Batch(name, tab, n, n)
    ml = _ml_buffer(tab["ml"], n, 0, 1)
    want = b.golden(tab["ml"])
    counts = DC.k10_counts(want, b.flags, n)
    K.ensemble(b.hdr, b.cfg, b.feat, b.X, ml, b.out, n, None)
    b.check(b.out, want, "no metrics")
    for launch in (1, 2):
        b.out.fill_(DC.RES_SENTINEL)
        K.ensemble(b.hdr, b.cfg, b.feat, b.X, ml, b.out, n, b.metrics)
        b.check(b.out, want, f"metrics launch {launch}")
        np.testing.assert_array_equal(b.metrics.cpu().numpy(), launch * counts)
    nan = np.isnan(tab["ml"]) & DC.k5_live(tab["flags"], n)     # NaN reached K5: the error score came out
    assert nan.any() and (_u32(b.out)[:n][nan, 1] == DC.bits([b.sc.ml_error_score])[0]).all()


@pytest.mark.parametrize("col,stride", DC.ML_LAYOUTS)
@pytest.mark.parametrize("live", ["all", "in_block", "none"])
def test_ensemble_kernel_ml_layout_and_dead_rows(col, stride, live):
    """ml_col / ml_stride with NaN in the columns not read; hdr.n below n_rows (inside a 256-row
    block and a 64-row tile) and 0: dead rows are zero records, rows past n_rows keep the sentinel."""
    K = _K()
    tab = DC.k5_table("default")
    n = len(tab["rule"])
    n_live = {"all": n, "in_block": n - 100, "none": 0}[live]
    assert live != "in_block" or (n_live % 256 and n_live % 64)
    b = Batch("default", tab, n, n_live, col, stride)
    want = b.golden(tab["ml"])
    K.ensemble(b.hdr, b.cfg, b.feat, b.X, _ml_buffer(tab["ml"], n, col, stride), b.out, n, b.metrics)
    b.check(b.out, want, f"col {col} stride {stride} live {n_live}")
    assert not want[n_live:].any() and (live == "none" or want[:n_live].any())
    np.testing.assert_array_equal(b.metrics.cpu().numpy(), DC.k10_counts(want, b.flags, n_live))


def test_ensemble_kernel_host_rows():
    """host_out: the pinned rows equal the device rows (dead rows zero). host_route: live rows
    land at base + p * stride + j * 8 of the region, dead rows are not written, and every other
    byte of the region keeps its sentinel; chunks of 100 rows end inside the 256-row blocks."""
    torch, K = _t(), _K()
    tab = DC.k5_table("default")
    n = len(tab["rule"])
    n_live = n - 100
    b = Batch("default", tab, n, n_live)
    ml = _ml_buffer(tab["ml"], n, 0, 1)
    want = b.golden(tab["ml"])
    host = torch.full((n + PAD, 2), DC.RES_SENTINEL, dtype=torch.int32).pin_memory()
    K.ensemble(b.hdr, b.cfg, b.feat, b.X, ml, b.out, n, b.metrics, host_out=host)
    torch.cuda.synchronize()
    b.check(b.out, want, "host_out: device rows")
    b.check(host, want, "host_out: pinned rows")
    # routed: C = 100 rows per chunk, chunks 864 B apart (64 B of padding each), 22 chunks
    C, stride = 100, 100 * 8 + 64
    P = -(-n // C)
    assert P >= 3 and 256 % C and stride % 8 == 0
    route = (np.arange(n, dtype=np.int64) * 7) % (P * C)       # 7 and P * C coprime: a permutation
    assert np.gcd(7, P * C) == 1 and len(set(route.tolist())) == n and route.max() < P * C
    region = torch.full((P * stride // 4,), DC.RES_SENTINEL, dtype=torch.int32).pin_memory()
    b.out.fill_(DC.RES_SENTINEL)
    K.ensemble(b.hdr, b.cfg, b.feat, b.X, ml, b.out, n, None,
               host_route=dict(base=region.data_ptr(), route=torch.from_numpy(route.astype(np.int32)).cuda(), C=C,
                               stride=stride))
    torch.cuda.synchronize()
    b.check(b.out, want, "host_route: device rows")
    exp = np.full(P * stride // 4, DC.RES_SENTINEL, np.uint32)
    live = DC.k5_live(b.flags, n_live)
    at = (route // C) * (stride // 4) + (route % C) * 2       # word offset of each row's record
    exp[at[live]], exp[at[live] + 1] = want[live, 0], want[live, 1]
    got = region.numpy().view(np.uint32)
    assert len(set((route[live] // C).tolist())) >= 3
    np.testing.assert_array_equal(got, exp)


# ------------------------------------------------------------------------------ K5 in the fused hosts
def _head(precision, k):
    from igaming_platform_amd.models.plan import HeadStep, Plan, to_device
    W1, b1, w2, b2 = DC.passthrough_head(k)
    hs = HeadStep(n1=W1.shape[0], k=k, act1="none", act2="none", w1_np=W1, b1_np=b1, w2_np=w2, b2=b2)
    to_device(Plan("t", k, [hs], 1, 0, {}, "input", "output"), "cuda", precision)
    return hs


def _reached(Y, ml, exact):
    """The model output the launch produced against the intended values. ``exact`` (f32 paths):
    equal - NaN stays NaN; an infinity may arrive as NaN (0 * inf in the other hidden units) and
    the denormal as 0, both still outside (0, 1); the bf16 head rounds, so only NaN is checked."""
    Y = np.asarray(Y, F32)
    nan = np.isnan(ml)
    assert np.isnan(Y[nan]).all()
    if not exact:
        return
    inf, den = np.isinf(ml), (ml != 0) & (np.abs(ml) < np.finfo(F32).tiny)
    rest = ~(nan | inf | den)
    np.testing.assert_array_equal(Y[rest], ml[rest])
    assert (np.isnan(Y[inf]) | (Y[inf] == ml[inf])).all()
    assert ((Y[den] == 0) | (Y[den] == ml[den])).all()


def _fused_case(host, live, via_m_ptr):
    """One fused launch and the standalone kernel over its model output: (a) records ==
    golden(own model output), (b) records and metric deltas == ensemble_kernel's. Returns the
    intended and the produced model outputs of the live rows."""
    torch, K = _t(), _K()
    R = DC.FUSED_ROWS
    trees = host.startswith("tree")
    tab = DC.k5_fused_rows("default", finite=trees)
    M = R if via_m_ptr else live                      # rows of the launch
    ens_rows = R if via_m_ptr else live               # the fused ensemble may not cover more rows than the launch
    if host == "tree_finish" and not via_m_ptr:
        ens_rows = R                                  # the finish kernel also covers ens rows past the tree's
    b = Batch("default", tab, ens_rows, live)
    m_ptr = torch.tensor([live], dtype=torch.int32, device="cuda") if via_m_ptr else None
    Y = D.sentinel_out(R + PAD, 1, torch.float32).cuda()
    ens = b.args(Y, metrics=True)
    if host.startswith("head"):
        precision, k = {"head_bf16": ("bf16", 32), "head_f32": ("fp32", 70), "head_f32_fast": ("fp32", 32)}[host]
        hs = _head(precision, k)
        assert D.head_dispatch(precision, hs.w1.shape[1], 64)[0] == {"head_bf16": "bf16", "head_f32": "generic",
                                                                      "head_f32_fast": "fast32"}[host]
        x = np.zeros((R, k), F32)
        x[:, 0] = tab["ml"]
        Xd = D.poisoned(R + PAD, M, k, k, torch.float32, x).cuda()
        K.mlp_head(hs, Xd, Y, M, m_ptr=m_ptr, ens=ens)
    else:
        k = 32 if host == "tree_head" else 1
        step, Xt = _forest(k)
        Xd = D.poisoned(R + PAD, M, 8, 8, torch.float32, Xt).cuda()
        groups = 4 if host == "tree_head" else 2
        slab = torch.full((groups * M * k,), float("nan"), device="cuda")
        if host == "tree_head":
            hs = _head("fp32", 32)
            assert K.tree_head_ok(step, hs, groups)
            cnt = torch.zeros(-(-M // 64), dtype=torch.int32, device="cuda")
            K.tree_head(step, hs, Xd, Y, M, slab, groups, cnt, m_ptr=m_ptr, ens=ens)
            assert int(cnt.abs().sum()) == 0
        else:
            K.tree_ensemble(step, Xd, Y, M, partial=slab, groups=groups, ens=ens)
    torch.cuda.synchronize()
    what = f"{host} live {live} {'m_ptr' if via_m_ptr else 'M'}"
    Yh = Y.cpu()
    assert D.untouched(Yh, live, 1), f"{what}: model output past the live rows"
    own = np.zeros(ens_rows, F32)
    own[:live] = Yh[:live, 0].numpy()
    _reached(own[:live], tab["ml"][:live], exact=host != "head_bf16")
    want = b.golden(own)
    b.check(b.out, want, what + " (a)")
    assert not want[live:].any()
    fused_metrics = b.metrics.cpu().numpy()
    np.testing.assert_array_equal(fused_metrics, DC.k10_counts(want, b.flags, live))
    alone = _res_out(ens_rows + PAD)
    b.metrics.zero_()
    K.ensemble(b.hdr, b.cfg, b.feat, b.X, torch.from_numpy(np.concatenate([own, np.full(PAD, np.nan, F32)])).cuda(),
               alone, ens_rows, b.metrics)
    torch.cuda.synchronize()
    assert torch.equal(alone, b.out), what + " (b)"
    np.testing.assert_array_equal(b.metrics.cpu().numpy(), fused_metrics)
    return tab["ml"][:live], own[:live]


@lru_cache(maxsize=None)
def _forest(k):
    """The lookup forest of the finite fused rows (K = 1: a regressor; K = 32: leaf vectors)."""
    from igaming_platform_amd.models.plan import Plan, compile_onnx, to_device
    from igaming_platform_amd.native import native
    tab = DC.k5_fused_rows("default", finite=True)
    trees, X = DC.lookup_forest(tab["ml"], k)
    case = TC.Case(f"lookup_k{k}", "complete", "reg", k, len(trees), DC.TREE_DEPTH, 8, (2,), ())
    (step,) = compile_onnx(native().OnnxModel.from_bytes(TC.make_model(case, trees).SerializeToString())).steps
    assert step.layout != "sparse" and step.depth == DC.TREE_DEPTH and step.k == k
    to_device(Plan("t", 8, [step], k, 0, {}, "input", "output"), "cuda")
    return step, X


FUSED_HOSTS = [(h, p) for h in ("head_bf16", "head_f32", "head_f32_fast", "tree_finish", "tree_head") for p in (False, True)
               if not (h == "tree_finish" and p)]   # the tree finish kernel has no m_ptr: its rows are the launch's


@pytest.mark.parametrize("host,via_m_ptr", FUSED_HOSTS, ids=[f"{h}-{'m_ptr' if p else 'M'}" for h, p in FUSED_HOSTS])
def test_fused_hosts_equal_golden_and_standalone(host, via_m_ptr):
    """Live counts of 1, 63, 64, 65 and 150 of 192 rows, as the launch's row count or through
    m_ptr with the ensemble covering all three tiles: the tiles without a live row take the
    hosts' own dead-row branch (the tree finish kernel: the ensemble rows past the tree's)."""
    nan_rows = 0
    for live in DC.FUSED_LIVE:
        ml, own = _fused_case(host, live, via_m_ptr)
        nan_rows += int((np.isnan(ml) & np.isnan(own)).sum())
    assert host.startswith("tree") or nan_rows > 0     # NaN reached K5 through the head kernels


# ------------------------------------------------------------------------------ K9 standalone
def _k9_dev():
    torch = _t()
    pf, ml, _ = DC.k9_table()
    return torch.from_numpy(pf).cuda(), torch.from_numpy(ml).cuda()


def _k9_check(out, want, rows, what):
    got = DC.bits(out.cpu().numpy())
    bad = np.nonzero((got[:rows] != DC.bits(want)).any(1))[0]
    assert not len(bad), f"{what}: {len(bad)} of {rows} rows differ, first {bad[:5]}: " \
                         f"{out.cpu().numpy()[bad[:3]]} != {np.asarray(want)[bad[:3]]}"
    assert D.untouched(out.cpu(), rows, 6), f"{what}: wrote past B"


@pytest.mark.parametrize("learned", [False, True], ids=["formula", "learned"])
def test_ltv_kernel_whole_table_and_block_edges(learned):
    torch, K = _t(), _K()
    pf, ml = _k9_dev()
    want = DC.k9_golden(learned)
    n = len(want)
    for B in (1, 25, 255, 256, 257, n):
        out = D.sentinel_out(B + PAD, 6, torch.float32).cuda()
        K.ltv(pf[:B].contiguous(), out, model_ltv=ml[:B].contiguous() if learned else None)
        _k9_check(out, want[:B], B, f"B {B}")


@pytest.mark.parametrize("learned", [False, True], ids=["formula", "learned"])
def test_ltv_kernel_through_slots(learned):
    """Slots with repeats, the table's last row and -1 (the empty profile's answer)."""
    torch, K = _t(), _K()
    pf, ml = _k9_dev()
    n = len(pf)
    rng = np.random.default_rng(31)
    slots = rng.integers(0, n, 700).astype(np.int32)
    slots[::13] = -1
    slots[5] = slots[6] = slots[300] = n - 1
    slots[7] = slots[8] = 0
    B = len(slots)
    mlv = DC.k9_table()[1][rng.integers(0, n, B)]
    want = np.array([DC.k9_row(DC.k9_predict(DC.k9_table()[0][s] if s >= 0 else np.zeros(25, F32),
                                             mlv[i] if learned else None)) for i, s in enumerate(slots)], F32)
    out = D.sentinel_out(B + PAD, 6, torch.float32).cuda()
    K.ltv(pf, out, model_ltv=torch.from_numpy(mlv).cuda() if learned else None,
          slots=torch.from_numpy(slots).cuda(), rows=B)
    _k9_check(out, want, B, "slots")
    assert (want[slots == -1] == DC.k9_zero(None)).all() or learned


# ------------------------------------------------------------------------------ K9 in the chain
EXT_W = 7
CHAIN_INSTANCES = [   # (width, split, env) -> the mlp_chain_kernel instance of launch_mlp_chain, all eight
    (64, False, {"IGP_MLP_ROWS": "16"}), (64, False, {"IGP_MLP_ROWS": "32"}), (64, False, {"IGP_MLP_ROWS": "64"}),
    (128, False, {"IGP_MLP_ROWS": "32"}), (128, False, {"IGP_MLP_ROWS": "64"}),
    (64, True, {}), (128, True, {"IGP_MLP_SPLIT_ROWS": "32"}), (128, True, {"IGP_MLP_SPLIT_ROWS": "64"}),
]


def _chain(width, split, zero):
    from igaming_platform_amd.models.plan import DenseStep, HeadStep
    rng = np.random.default_rng(600 + width)
    k0 = 25 + EXT_W
    def w(scale, *shape):
        return np.zeros(shape, F32) if zero else rng.normal(0, scale, shape).astype(F32)
    steps = [DenseStep(n=width, k=k0, act="relu", w_np=w(0.3, width, k0), b_np=w(0.1, width)),
             HeadStep(n1=width, k=width, act1="relu", act2="none", w1_np=w(0.2, width, width), b1_np=w(0.1, width),
                      w2_np=w(40.0, width), b2=0.0 if zero else 300.0)]
    pk = _K().MlpChainPack(steps, "cuda", split=split)
    assert pk.waves() == (8 if width == 128 else 4)
    return pk


@lru_cache(maxsize=None)
def _learned_cases():
    """(profiles [R, 25] - one per churn value of the table, values [V] - every learned LTV of the
    learned block, golden [V, R + 1, 6] - the last row of each: an empty profile)."""
    pf, ml, blocks = DC.k9_table()
    lo, hi = blocks["learned"]
    prof, seen = [], set()
    for r in pf[lo:hi]:
        if r.tobytes() not in seen:
            seen.add(r.tobytes())
            prof.append(r)
    vals = sorted(set((ml[lo:hi] + F32(0)).tolist()))   # +0.0 for -0.0: 0 (the chain's sum) + b2 cannot be -0.0
    zero = np.zeros(25, F32)
    gold = np.array([[DC.k9_row(DC.k9_predict(r, v)) for r in prof + [zero]] for v in vals], F32)
    return np.array(prof, F32), np.array(vals, F32), gold


@pytest.mark.parametrize("width,split,env", CHAIN_INSTANCES,
                         ids=[f"w{w}-{'split' if s else 'bf16'}-{'-'.join(e.values()) or 'default'}" for w, s, e in CHAIN_INSTANCES])
def test_chain_ltv_epilogue_equals_golden_on_its_own_ml(width, split, env, monkeypatch):
    """The gather + chain + K9 kernel: ltv_out == golden(profile of the slot, the launch's own
    ml), -1 slots as the empty profile, a live count inside a tile through m_ptr, rows past it
    untouched; its ml bit-equal to a dense launch over ltv_assemble's rows; and zero-weight chains
    whose b2 is each learned-mode threshold value (ml == b2) over one profile per churn value."""
    torch, K = _t(), _K()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pf_np = DC.k9_table()[0]
    pf, _ = _k9_dev()
    n = len(pf_np)
    rng = np.random.default_rng(77)
    ext_np = rng.normal(0, 1, (n, EXT_W)).astype(F32)
    ext = torch.from_numpy(ext_np).cuda()
    rows, live = 300, 277
    assert live % 16 and live % 32 and live % 64
    slots_np = rng.integers(0, n, rows).astype(np.int32)
    slots_np[::17] = -1
    slots_np[3] = n - 1
    slots = torch.from_numpy(slots_np).cuda()
    m_ptr = torch.tensor([live], dtype=torch.int32, device="cuda")
    pk = _chain(width, split, zero=False)
    ml = D.sentinel_out(rows + PAD, 1, torch.float32).cuda().view(-1)
    out = D.sentinel_out(rows + PAD, 6, torch.float32).cuda()
    K.mlp_chain(pk, rows, slots=slots, pf_tab=pf, ext_tab=ext, ml=ml, ltv_out=out, m_ptr=m_ptr)
    torch.cuda.synchronize()
    mlh = ml.cpu().numpy()
    assert (mlh[live:] == D.SENTINEL).all() and np.isfinite(mlh[:live]).all()
    want = np.array([DC.k9_row(DC.k9_predict(pf_np[s] if s >= 0 else np.zeros(25, F32), mlh[i]))
                     for i, s in enumerate(slots_np[:live])], F32)
    _k9_check(out, want, live, "gather launch")
    assert len(set(want[:, 4].tolist())) >= 3          # the random chain's LTVs spread over the segments
    Xa = D.sentinel_out(rows + PAD, 25 + EXT_W, torch.float32).cuda()
    K.ltv_assemble(slots, pf, ext, Xa, rows, m_ptr=m_ptr)
    ml2 = D.sentinel_out(rows + PAD, 1, torch.float32).cuda().view(-1)
    K.mlp_chain(pk, rows, X=Xa, ml=ml2, m_ptr=m_ptr)
    torch.cuda.synchronize()
    assert torch.equal(ml, ml2), "gather launch vs dense launch over ltv_assemble"
    # the segment thresholds: one launch per learned LTV, b2 = the value
    prof, vals, gold = _learned_cases()
    R = len(prof) + 1
    assert 16 < R < 32
    tab = torch.from_numpy(prof).cuda()
    ext0 = torch.zeros((len(prof), EXT_W), device="cuda")
    sl = torch.tensor(list(range(R - 1)) + [-1] + [0] * (32 - R), dtype=torch.int32, device="cuda")
    mp = torch.tensor([R], dtype=torch.int32, device="cuda")
    zk = _chain(width, split, zero=True)
    mls = D.sentinel_out(len(vals), 32, torch.float32).cuda()
    outs = D.sentinel_out(len(vals) * 32, 6, torch.float32).cuda().view(len(vals), 32, 6)
    for i, v in enumerate(vals):
        zk.b2 = float(v)    # K.mlp_chain reads the pack's b2 at every launch; "ml != b2" below fails if that changes
        K.mlp_chain(zk, 32, slots=sl, pf_tab=tab, ext_tab=ext0, ml=mls[i], ltv_out=outs[i], m_ptr=mp)
    torch.cuda.synchronize()
    mlh, oh = mls.cpu().numpy(), outs.cpu().numpy()
    assert (DC.bits(mlh[:, :R]) == DC.bits(vals)[:, None]).all(), "ml != b2"
    assert (mlh[:, R:] == D.SENTINEL).all() and (oh[:, R:] == D.SENTINEL).all()
    bad = np.argwhere((DC.bits(oh[:, :R]) != DC.bits(gold)).any(2))
    assert not len(bad), f"{len(bad)} (value, profile) pairs differ, first {bad[:3]}: " \
                         f"{[(vals[i], oh[i, j], gold[i, j]) for i, j in bad[:3]]}"


# ------------------------------------------------------------------------------ ltv_assemble
@pytest.mark.parametrize("ext_w,x_w,rows,live", [(7, 32, 37, 30), (0, 25, 11, None), (3, 41, 300, 277), (7, 32, 64, 0)])
def test_ltv_assemble_against_float64(ext_w, x_w, rows, live):
    """sign(x) log1p|x| of the profile columns at the project's f32-vs-float64 tolerance, the ext
    columns bit for bit, columns past 25 + ext_w and -1 / dead rows zero, everything at or past
    n_rows NaN as before; n_rows * x_w is no multiple of 256 in the first three shapes."""
    torch, K = _t(), _K()
    rng = np.random.default_rng(40 + x_w)
    cap = 64
    pf_np = DC.k9_table()[0][rng.integers(0, len(DC.k9_table()[0]), cap)].copy()
    pf_np[0, :len(DC.ASSEMBLE_VALUES)] = DC.ASSEMBLE_VALUES
    pf_np[1] = pf_np[0][::-1]
    ext_np = rng.normal(0, 1, (cap, max(ext_w, 1))).astype(F32)
    ext_np[0, 0] = -0.0
    slots_np = rng.integers(0, cap, rows).astype(np.int32)
    slots_np[:4] = (0, 1, -1, cap - 1)
    n_live = rows if live is None else live
    X = torch.full((rows + PAD, x_w), float("nan"), device="cuda")
    K.ltv_assemble(torch.from_numpy(slots_np).cuda(), torch.from_numpy(pf_np).cuda(),
                   torch.from_numpy(ext_np).cuda() if ext_w else None, X, rows,
                   m_ptr=None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda"))
    got = X.cpu().numpy()
    assert np.isnan(got[rows:]).all()
    ok = (np.arange(rows) < n_live) & (slots_np >= 0)
    assert not DC.bits(got[:rows][~ok]).any()                                 # +0.0, bit for bit
    s = slots_np[ok]
    np.testing.assert_allclose(got[:rows][ok, :25].astype(np.float64), DC.ref_log1p(pf_np[s]), rtol=1e-5, atol=1e-5)
    assert (np.signbit(got[:rows][ok, :25]) == np.signbit(pf_np[s])).all()    # -0.0 stays -0.0
    if ext_w:
        assert (DC.bits(got[:rows][ok, 25:25 + ext_w]) == DC.bits(ext_np[s, :ext_w])).all()
    assert not DC.bits(got[:rows][:, 25 + ext_w:]).any()


# ------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("b", DC.ENGINE_B)
def test_gpu_engine_with_a_constant_model_matches_golden_ensemble(b):
    from tests.test_decision_edges import engine_vs_golden
    from tests.test_engine_gpu import NOW

    def tune(cfg):
        cfg.gpu.buckets = [64]
        cfg.gpu.max_batch = 64
    engine_vs_golden("gpu", b, NOW, tune=tune, capacity=4096)
