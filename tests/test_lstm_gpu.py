"""K4 fused LSTM kernel (csrc/kernels/lstm.hip) vs the C++ CPU executor (fp32 ONNX LSTM semantics)
and a float64 reference. Shapes: rows 1 / 17 / 100 (partial tile, two tiles, many tiles), H = 64
with one layer up to H = 256 with two (the widest instantiation)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODELS = [
    dict(seq=12, hidden=64, layers=1, head=False),
    dict(seq=16, hidden=128, layers=2, head=True, in_dim=40),
    dict(seq=20, hidden=256, layers=2, head=True),
]
DIRECTIONS = [
    dict(seq=12, hidden=128, layers=2, direction="reverse"),
    dict(seq=16, hidden=128, layers=1, direction="bidirectional"),
    dict(seq=12, hidden=64, layers=2, layout=1),
    dict(seq=12, hidden=64, layers=1, direction="bidirectional", layout=1),
]
REF_ROWS = 100


def _ids(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(N, model, X [T, 100, I], executor output [100, ...]) of a builder model: computed once and
    shared; rows are independent sequences, so a test on fewer rows reads a prefix."""
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    kw = dict(key)
    N = native()
    m = N.OnnxModel.from_bytes(builders.build("lstm", **kw).SerializeToString())
    X = np.random.default_rng(len(key) + kw["hidden"]).standard_normal(
        (kw["seq"], REF_ROWS, kw.get("in_dim", 16))).astype(np.float32)
    feed = np.ascontiguousarray(X.transpose(1, 0, 2)) if kw.get("layout") else X
    ref = N.Executor(m).run({"input": feed})["output"]
    X.setflags(write=False)
    ref.setflags(write=False)
    return N, m, X, ref


def _run(kw, rows, precision):
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel, LstmModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    N, m, X, ref = _reference(tuple(sorted(kw.items())))
    plan = to_device(compile_onnx(m), "cuda", precision)
    dm = DeviceModel(plan, "cuda", [rows])
    assert isinstance(dm.gru, LstmModel) and dm.gru.split == (precision == "fp32")
    x = np.array(X[:, :rows])  # a writable copy (the shared reference stays read-only)
    feed = np.ascontiguousarray(x.transpose(1, 0, 2)) if kw.get("layout") else x
    got = dm.run(torch.from_numpy(feed).cuda(), rows)[:rows].cpu().numpy()
    want = ref[:rows]
    return got.reshape(want.shape), want


@pytest.mark.parametrize("rows", [1, 17, 100])
@pytest.mark.parametrize("kw", MODELS, ids=_ids)
def test_lstm_fp32_plan_matches_executor(kw, rows):
    got, ref = _run(kw, rows, "fp32")
    err = float(np.abs(got - ref).max())
    print(f"lstm split vs executor {_ids(kw)} rows {rows}: max err {err:.3e}")
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4)


@pytest.mark.parametrize("kw", MODELS, ids=_ids)
def test_lstm_bf16_plan_matches_executor(kw):
    got, ref = _run(kw, 100, "bf16")
    err = np.abs(got - ref)
    print(f"lstm bf16 vs executor {_ids(kw)}: max err {err.max():.3e} mean {err.mean():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-2)
    assert err.mean() < 2e-3


@pytest.mark.parametrize("rows", [7, 100])
@pytest.mark.parametrize("kw", DIRECTIONS, ids=_ids)
def test_lstm_directions_and_layout_match_executor(kw, rows):
    """reverse (the kernel reads the sequence last step first), bidirectional (a forward and a
    reverse launch + the head over [N, 2H]) and layout-1 models, split numerics."""
    got, ref = _run(kw, rows, "fp32")
    err = float(np.abs(got - ref).max())
    print(f"lstm split vs executor {_ids(kw)} rows {rows}: max err {err:.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4)


def _ring_store(T):
    """A DeviceFeatureStore (ring of T + 8 events) whose first accounts hold 0, 3, exactly T and
    more than T (wrapped) events; returns (store, bf16-exact ring contents, rt rows)."""
    import torch
    from igaming_platform_amd.config import FeatureConfig
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.layouts import ACCTRT
    fc = FeatureConfig()
    fc.event_ring = T + 8
    C, R, D = 12, fc.event_ring, fc.event_dim
    store = DeviceFeatureStore(C, fc, "cuda", events=True, max_events=64)
    rng = np.random.default_rng(2)
    ev_bf = torch.from_numpy(rng.standard_normal((C, R, D)).astype(np.float32)).to(torch.bfloat16)
    store.ev.copy_(ev_bf.view(torch.int16).cuda())
    rt = np.zeros(C, ACCTRT)
    rt["ev_head"] = rng.integers(0, R, C)
    rt["ev_count"] = rng.integers(0, R + 1, C)
    rt["ev_count"][:5] = [0, 3, T, R, T + 3]
    rt["ev_head"][:5] = [0, 3, T, 5, 2]   # accounts 3 and 4 have wrapped round the ring
    store.rt.copy_(torch.from_numpy(rt.view(np.int32).reshape(C, -1).copy()).cuda())
    return store, ev_bf.float().numpy(), rt


def _unroll(evq, rt, slots, T):
    """Host gather of the kernel's event-ring input: oldest first, right-aligned, zeros before."""
    R = evq.shape[1]
    X = np.zeros((T, len(slots), evq.shape[2]), np.float32)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        cnt, head = min(int(rt["ev_count"][s]), T), int(rt["ev_head"][s])
        for t in range(T - cnt, T):
            X[t, b] = evq[s, (head - T + t) % R]
    return X


@pytest.mark.parametrize("split,atol", [(True, 1e-4), (False, 1e-2)])
def test_lstm_event_ring_input_matches_executor(split, atol):
    import torch
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    from igaming_platform_amd.ops import kernels as K
    T = 16
    N = native()
    m = N.OnnxModel.from_bytes(builders.build("lstm", seq=T, hidden=128, layers=2).SerializeToString())
    plan = to_device(compile_onnx(m), "cuda")
    store, evq, rt = _ring_store(T)
    slots = np.array([0, 1, 2, 3, 4, -1, 7, 3, 11, -1, 5, 6, 8, 9, 10, 1, 2, 4, 0], np.int32)
    rows = len(slots)
    ref = N.Executor(m).run({"input": _unroll(evq, rt, slots, T)})["output"].reshape(-1)
    lp = K.LstmPack([s for s in plan.steps if s.kind == "lstm"], plan.steps[-1], "cuda", split=split)
    out = torch.full((rows,), -9.0, dtype=torch.float32, device="cuda")
    K.lstm(lp, rows, T, out=out, store=store, slots=torch.from_numpy(slots).cuda())
    got = out.cpu().numpy()
    print(f"lstm event rings split={split}: max err {np.abs(got - ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    # an empty history (no slot, or no events) scores as the all-zero sequence
    assert got[5] == got[9] == got[0] == got[18]


def test_lstm_respects_live_rows():
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    m = native().OnnxModel.from_bytes(builders.build("lstm", seq=8, hidden=64, layers=1).SerializeToString())
    dm = DeviceModel(to_device(compile_onnx(m), "cuda"), "cuda", [64])
    X = torch.randn(8, 64, 16, device="cuda")
    dm.out.fill_(-7.0)
    n = torch.tensor([20], dtype=torch.int32, device="cuda")  # ends inside the second workgroup
    dm.run(X, 64, m_ptr=n)
    o = dm.out.cpu().numpy().reshape(-1)
    assert np.all(o[20:] == -7.0) and np.all(o[:20] != -7.0)
    # the same for the final states of a headless model
    from igaming_platform_amd.ops import kernels as K
    plan = compile_onnx(native().OnnxModel.from_bytes(
        builders.build("lstm", seq=8, hidden=64, layers=1, head=False).SerializeToString()))
    lp = K.LstmPack(plan.steps, None, "cuda", split=True)
    yh = torch.full((64, 64), 5.0, device="cuda")
    K.lstm(lp, 64, 8, yh=yh, X=X, m_ptr=n)
    assert bool(torch.all(yh[20:] == 5.0)) and bool(torch.all(yh[:20] != 5.0))


def test_lstm_32_row_tiles_match_16():
    """32 rows per workgroup (two row tiles share every streamed weight fragment; only where the
    LDS formula allows) equal the 16-row kernel bit for bit, with a batch that ends inside a
    workgroup: split at H = 256 (the largest LDS footprint) and bf16 at H = 64."""
    import torch
    from igaming_platform_amd.models.plan import compile_onnx
    from igaming_platform_amd.native import hipk
    from igaming_platform_amd.ops import kernels as K
    for kw, split in ((MODELS[2], True), (MODELS[0], False)):
        N, m, X, _ = _reference(tuple(sorted(kw.items())))
        plan = compile_onnx(m)
        cells = [s for s in plan.steps if s.kind == "lstm"]
        head = plan.steps[-1] if kw["head"] else None
        lp = K.LstmPack(cells, head, "cuda", split=split)
        assert hipk().lstm_tile_rows(lp.H, lp.layers[0]["kx_pad"], int(split), 32) == 32
        Xd = torch.from_numpy(X.copy()).cuda()
        outs = {}
        for tile in (16, 32):
            o = torch.full((REF_ROWS, 1 if head else lp.H), -9.0, device="cuda")
            K.lstm(lp, REF_ROWS, kw["seq"], X=Xd, tile_rows=tile, **({"out": o} if head else {"yh": o}))
            outs[tile] = o.cpu().numpy()
        assert np.all(np.isfinite(outs[32])) and np.all(outs[32] != -9.0)
        np.testing.assert_array_equal(outs[16], outs[32])


def _lstm_f64(plan, X):
    """Plain PyTorch float64 loop over the plan's ONNX LSTM stack (+ N=1 head), gate order
    i, o, f, c as in the ONNX spec; X [T, rows, I] numpy."""
    import torch
    cells = [s for s in plan.steps if s.kind == "lstm"]
    head = [s for s in plan.steps if s.kind != "lstm"]
    x = torch.from_numpy(X).double()
    for g in cells:
        H = g.hidden
        W, R, B = (torch.from_numpy(np.asarray(a, np.float64)) for a in (g.w_np, g.r_np, g.b_np))
        h = torch.zeros(x.shape[1], H, dtype=torch.float64)
        c = torch.zeros_like(h)
        xw = x @ W.T + B[:4 * H] + B[4 * H:]
        ys = []
        for t in range(x.shape[0]):
            a = xw[t] + h @ R.T
            c = torch.sigmoid(a[:, 2 * H:3 * H]) * c + torch.sigmoid(a[:, :H]) * torch.tanh(a[:, 3 * H:])
            h = torch.sigmoid(a[:, H:2 * H]) * torch.tanh(c)
            ys.append(h)
        x = torch.stack(ys)
    y = x[-1]
    if head:
        hd = head[0]
        y = y @ torch.from_numpy(np.asarray(hd.w_np, np.float64)).T
        if hd.b_np is not None:
            y = y + torch.from_numpy(np.asarray(hd.b_np, np.float64))
        if hd.act == "sigmoid":
            y = torch.sigmoid(y)
    return y.reshape(-1).numpy()


def test_lstm_split_mode_fp32_faithful_over_100_steps():
    """A 2 x 256 LSTM over 100 steps + Gemm/Sigmoid head at 64 rows against a float64 PyTorch
    loop: the split mode (fp32 plan) stays within 1e-4 and under a tenth of the bf16 plan's error
    (the GRU test's bounds). The float64 loop itself is checked against the fp32 executor on 8 rows."""
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    N = native()
    m = N.OnnxModel.from_bytes(builders.build("lstm", seq=100, in_dim=16, hidden=256, layers=2).SerializeToString())
    plan32 = to_device(compile_onnx(m), "cuda", "fp32")
    plan16 = to_device(compile_onnx(m), "cuda", "bf16")
    rows = 64
    X = np.random.default_rng(41).standard_normal((100, rows, 16)).astype(np.float32)
    small = N.Executor(m).run({"input": np.ascontiguousarray(X[:, :8])})["output"].reshape(-1)
    np.testing.assert_allclose(_lstm_f64(plan32, X[:, :8]), small, rtol=0, atol=2e-6)
    # a head that spreads the scores over (0, 1) (random init puts them all near 0.5)
    for p in (plan32, plan16):
        p.steps[-1].w_np = p.steps[-1].w_np * 40.0
    ref = _lstm_f64(plan32, X)
    Xd = torch.from_numpy(X).cuda()
    outs = {}
    for name, plan in (("split", plan32), ("bf16", plan16)):
        dm = DeviceModel(plan, "cuda", [rows])
        assert dm.gru.split == (name == "split")
        outs[name] = dm.run(Xd, rows)[:rows].reshape(-1).cpu().numpy().copy()
    e_split = float(np.abs(outs["split"] - ref).max())
    e_bf16 = float(np.abs(outs["bf16"] - ref).max())
    print(f"lstm 2x256 T=100: split err {e_split:.3e}, bf16 err {e_bf16:.3e}, score spread {np.ptp(ref):.3f}")
    assert e_split <= 1e-4, (e_split, e_bf16)
    assert e_split < e_bf16 / 10, (e_split, e_bf16)


def test_abuse_gpu_with_lstm_plan_matches_direct_run():
    """AbuseGpu (captured graph per bucket, H2D slots -> fused LSTM + head over the event rings
    -> D2H) returns what a direct LstmModel.run gives for the same slots."""
    import torch
    from igaming_platform_amd.engine.abuse import AbuseGpu
    from igaming_platform_amd.engine.runner import LstmModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    T = 16
    m = native().OnnxModel.from_bytes(builders.build("lstm", seq=T, hidden=64, layers=2).SerializeToString())
    plan = to_device(compile_onnx(m), "cuda")
    store, _, _ = _ring_store(T)
    ag = AbuseGpu(store, plan, buckets=(64,), use_graphs=True)
    assert isinstance(ag.gm, LstmModel) and ag.T == T
    ag.capture()
    assert ag.graphs
    slots = np.array([0, 1, 2, 3, 4, 5, 11, 3, 7, 1, 9, 10, 6, 8, 2, 4, 0, 3, 5, 7], np.int32)
    got = ag.score_slots(slots)
    lm = LstmModel(plan.steps, "cuda", True, 64)
    out = torch.full((64,), -9.0, device="cuda")
    lm.run(len(slots), T, out, store=store, slots=torch.from_numpy(slots).cuda())
    want = out[:len(slots)].cpu().numpy()
    assert np.all(want != -9.0) and len(set(want.tolist())) > 5
    np.testing.assert_array_equal(got, want)


def test_risk_engine_gpu_lstm_abuse_model_matches_cpu_backend():
    """An ONNX file from builders.build("lstm") as ``abuse_model``: CheckBonusAbuse on
    backend="gpu" (fp32 plan: split kernel over the HBM event rings) against backend="cpu" (the
    C++ executor over the same encoded events), accounts with 5, 30 and more than 100 events and
    one without any. Tolerance: the split mode's figure against the executor, 1e-4."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.layouts import ACCTBATCH
    from igaming_platform_amd.onnx import builders
    now = 1_760_000_000
    m = builders.build("lstm", seq=100, hidden=64, layers=2).SerializeToString()
    cfg = Config()
    cfg.gpu.buckets = [64]
    cfg.gpu.max_batch = 64
    g = RiskEngine(cfg, backend="gpu", capacity=256, abuse_model=m)
    c = RiskEngine(cfg, backend="cpu", capacity=256, abuse_model=m)
    rows = np.zeros(1, ACCTBATCH)
    rows["present"] = 1
    ev = [dict(account_id=a, amount=100 * (i % 13) + 1, transaction_type=["deposit", "bet", "win"][i % 3],
               device_id=f"d{i % 3}", ts=now - 500 + i)
          for a, n in (("few", 5), ("some", 30), ("many", 130)) for i in range(n)]
    for e in (g, c):
        e.load_batch_features(["none"], rows)
        e.ingest_events(ev)
    ids = ["none", "few", "some", "many"]
    rg, rc = g.check_bonus_abuse_batch(ids, now=now), c.check_bonus_abuse_batch(ids, now=now)
    got = np.array([r.model_score for r in rg])
    want = np.array([r.model_score for r in rc])
    print(f"lstm abuse model gpu vs cpu backend: {got} vs {want}")
    assert len(set(np.round(want, 5))) == 4
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
