"""Temporal convolutions on the device (csrc/kernels/conv1d.hip): integer layers bit-equal to the
float64 reference over the shape grid, the epilogue, integer and real-valued builder models on
DeviceModel, the wrappers' argument checks, AbuseGpu and the engine. Cases, reference and tolerance:
tests/tcn_cases.py."""
import numpy as np
import pytest

from tests import tcn_cases as C

pytestmark = pytest.mark.gpu

CANARY = -7.0
ACTS = ("none", "relu", "sigmoid", "tanh")
EPS32 = float(np.finfo(np.float32).eps)


def make_step(w, b, dil, pad_left, T, act="none", act_post="none", res=None):
    """An uploaded ConvStep from ONNX-shaped weights w [M, C, k]."""
    from igaming_platform_amd.models.plan import ConvStep, check_conv, conv_tables
    s = ConvStep(c_in=w.shape[1], c_out=w.shape[0], k=w.shape[2], dil=dil, pad_left=pad_left,
                 w_np=np.ascontiguousarray(w.transpose(0, 2, 1), np.float32), b_np=np.ascontiguousarray(b, np.float32),
                 act=act, act_post=act_post, res=res, seq=T)
    check_conv(s)
    t = conv_tables(s)
    s.w, s.b = t["w"].cuda(), t["bias"].cuda()
    return s


def seq_buf(x, alloc=None, fill=1e30):
    """x [rows, T, C] in a garbage-filled channel-last device buffer [alloc, T, round_up(C, 4) + 4]."""
    import torch
    rows, T, Cn = x.shape
    buf = torch.full((alloc or rows + 2, T, -(-Cn // 4) * 4 + 4), fill, dtype=torch.float32)
    buf[:rows, :, :Cn] = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return buf.cuda()


def run_conv(s, x, dense=False, res=None, m_ptr=None, n_rows=None, alloc=None, **kw):
    """K.conv1d on x [rows, T, C] (as an activation buffer, or as the dense model input [T, rows, C])
    into a canary-filled output; returns it on the host, [alloc, T, ld]."""
    import torch
    from igaming_platform_amd.ops import kernels as K
    rows, T, _ = x.shape
    alloc = alloc or rows + 2
    Y = torch.full((alloc, T, -(-s.c_out // 4) * 4 + 4), CANARY, dtype=torch.float32).cuda()
    src = (dict(X=torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2), np.float32)).cuda()) if dense
           else dict(A=seq_buf(x, alloc)))
    K.conv1d(s, rows if n_rows is None else n_rows, T, Y, res=None if res is None else seq_buf(res, alloc),
             m_ptr=m_ptr, **src, **kw)
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def ref_layer(x, w, b, dil, pad_left, act="none", act_post="none", res=None):
    """[rows, T, C] -> [rows, T, M] in float64, the ConvStep formula."""
    y = C.ref_act(C.ref_conv(x.transpose(0, 2, 1), w, b, dil, pad_left), act)
    if res is not None:
        y = y + res.transpose(0, 2, 1)
    return C.ref_act(y, act_post).transpose(0, 2, 1)


# ------------------------------------------------------------------------------ the shape grid, exact
def test_integer_layers_bit_equal_over_the_grid():
    """One integer layer per sampled grid case (every listed T, C_in, C_out, k, d, pad_left and row
    count appears): the device equals the float64 reference bit for bit, from an activation buffer and
    from the dense model input; nothing is stored past the rows or the last 16-channel block."""
    cases = C.grid_sample()
    for dim, want in ((0, {1, 2, 15, 16, 17, 100}), (1, {1, 3, 16, 17}), (2, {1, 15, 16, 17, 33}), (3, {1, 2, 3}),
                      (5, {"zero", "causal", "half"}), (6, {1, 63, 65})):
        assert want <= {c[dim] for c in cases}, (dim, cases)
    assert {1, 2, 4} <= {c[4] for c in cases} and any(c[4] * (c[3] - 1) >= c[0] for c in cases), cases
    rng = np.random.default_rng(17)
    for i, (T, ci, co, k, d, pad, rows) in enumerate(cases):
        x, w, b = C.int_conv_case(rng, rows, T, ci, co, k, d)
        pl = C.pad_of(pad, k, d)
        ref = ref_layer(x, w, b, d, pl)
        assert np.abs(ref).max() < 2 ** 24
        Y = run_conv(make_step(w, b, d, pl, T), x, dense=bool(i & 1))
        what = f"case {i} {(T, ci, co, k, d, pad, rows)} of {cases}"
        assert np.array_equal(Y[:rows, :, :co].astype(np.float64), ref), what
        assert (Y[rows:] == CANARY).all() and (Y[:, :, -(-co // 16) * 16:] == CANARY).all(), what
        assert (Y[:rows, :, co:-(-co // 16) * 16] == 0).all(), what


# ------------------------------------------------------------------------------ the epilogue
@pytest.mark.parametrize("with_res", [False, True])
def test_every_activation_pair(with_res):
    """bias -> act -> + res -> act_post for all 16 pairs. Pairs of none / relu are exact on integer
    data; sigmoid / tanh stages are compared within 8 f32 epsilons of max(1, |value|): expf / tanhf are
    good to 2 ulp each, there are at most two such stages with slope <= 1, plus the roundings of the sum."""
    rng = np.random.default_rng(5)
    rows, T, ci, co, k, d = 3, 17, 5, 19, 3, 2
    x, w, b = C.int_conv_case(rng, rows, T, ci, co, k, d)
    w = np.sign(w) * (rng.random(w.shape) < 0.4)     # small sums: the transcendental stages are not saturated
    res = rng.integers(-3, 4, (rows, T, co)).astype(np.float32) if with_res else None
    for act in ACTS:
        for post in ACTS:
            s = make_step(w, b, d, 4, T, act=act, act_post=post, res=0 if with_res else None)
            got = run_conv(s, x, res=res)[:rows, :, :co].astype(np.float64)
            ref = ref_layer(x, w, b, d, 4, act, post, res)
            if {act, post} <= {"none", "relu"}:
                assert np.array_equal(got, ref), (act, post)
            else:
                err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
                print(f"act {act} act_post {post} res {with_res}: max err {err.max() / EPS32:.2f} eps")
                assert err.max() <= 8 * EPS32, (act, post, float(err.max()))


# ------------------------------------------------------------------------------ builder models on DeviceModel
def _device_model(m, bucket=64):
    from igaming_platform_amd.engine.runner import DeviceModel, TcnModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    plan = to_device(compile_onnx(native().OnnxModel.from_bytes(m.SerializeToString())), "cuda")
    dm = DeviceModel(plan, "cuda", [bucket])
    assert isinstance(dm.gru, TcnModel)
    return dm


def _run_model(dm, X, layout, bucket=64):
    import torch
    n = X.shape[0] if layout else X.shape[1]
    shape = (bucket,) + X.shape[1:] if layout else (X.shape[0], bucket, X.shape[2])
    Xd = torch.zeros(shape, dtype=torch.float32)
    if layout:
        Xd[:n] = torch.from_numpy(X)
    else:
        Xd[:, :n] = torch.from_numpy(X)
    out = dm.run(Xd.cuda(), bucket)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy().astype(np.float64)


INT_KW = dict(seq=20, in_dim=5, channels=(8, 8), dilations=(1, 2), head=False, weights=C.int_weights(-1, 1))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("style,readout", [("pads", "last"), ("chomp", "max"), ("pad_op", "last")])
def test_integer_models_bit_equal(style, readout, layout):
    """Whole integer networks (two residual blocks; the second block's residual is read from the
    first block's output, two steps back, the first one's through a k = 1 convolution) on DeviceModel:
    bit-equal to float64, every partial sum being below 2^24 (tcn_cases.int_bound)."""
    kw = dict(INT_KW, style=style, readout=readout, layout=layout)
    m = C.builders.tcn(**kw)
    rng = np.random.default_rng(2)
    X = rng.integers(-2, 3, (9, 20, 5) if layout else (20, 9, 5)).astype(np.float32)
    assert C.int_bound(m, X, **kw) < 2 ** 24
    dm = _device_model(m)
    assert [s.res for s in dm.plan.steps if s.kind == "conv"] == [None, None, 1, None, 2]
    ref = C.ref_tcn(m, X, **kw)
    assert np.ptp(ref) > 0
    assert np.array_equal(_run_model(dm, X, layout), ref)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name", sorted(C.REAL_MODELS))
def test_real_models_against_executor_and_float64(name, layout):
    """The builder's defaults and the 64-channel x 4-block model on DeviceModel: within REAL_TOL (derived
    from the float32 reference evaluation, tcn_cases.py) of the float64 reference and of the executor."""
    from igaming_platform_amd.native import native
    kw = dict(C.REAL_MODELS[name], layout=layout)
    m = C.builders.tcn(**kw)
    X = C.real_input(layout, seq=kw.get("seq", 100))
    got = _run_model(_device_model(m), X, layout)
    ref = C.ref_tcn(m, X, **kw)
    exe = native().Executor(native().OnnxModel.from_bytes(m.SerializeToString())).run({"input": X})["output"].astype(np.float64)
    e_ref, e_exe = float(np.abs(got - ref).max()), float(np.abs(got - exe).max())
    print(f"tcn {name} layout {layout}: device vs float64 {e_ref:.3e}, vs executor {e_exe:.3e}, tolerance {C.REAL_TOL:.1e}, "
          f"score spread {np.ptp(ref):.3f}")
    assert np.ptp(ref) > 1e-3
    assert e_ref <= C.REAL_TOL and e_exe <= C.REAL_TOL, (e_ref, e_exe)


# ------------------------------------------------------------------------------ argument checks
def test_wrappers_refuse_bad_arguments_before_launching():
    import torch
    from dataclasses import replace
    from igaming_platform_amd.ops import kernels as K
    rng = np.random.default_rng(0)
    x, w, b = C.int_conv_case(rng, 4, 16, 8, 8, 3, 1)
    s = make_step(w, b, 1, 2, 16)
    A, Y = seq_buf(x), torch.zeros((6, 16, 8), device="cuda")
    X = torch.zeros((16, 6, 8), device="cuda")
    bad = [
        dict(Y=Y.double(), A=A), dict(Y=Y[:, :, :6], A=A), dict(Y=Y.cpu(), A=A), dict(Y=Y, A=A.half()),
        dict(Y=Y, A=A[:, :8]), dict(Y=Y, A=Y), dict(Y=Y, A=A, X=X), dict(Y=Y), dict(Y=Y, A=A, res=Y),
        dict(Y=Y, X=X[:, :, :7]), dict(Y=Y, X=X[:8]), dict(Y=Y, A=A, tt=48), dict(Y=Y, A=A, m_ptr=torch.zeros(1, device="cuda")),
        dict(Y=Y, A=A, n_rows=7), dict(Y=Y, A=A, T=2000),
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            K.conv1d(s, kw.pop("n_rows", 4), kw.pop("T", 16), kw.pop("Y"), **kw)
    for st in (replace(s, w=None), replace(s, w=s.w[:1, :1]), replace(s, pad_left=3), replace(s, act="gelu"),
               replace(s, dil=200), replace(s, k=9), replace(s, res=0)):
        with pytest.raises(ValueError):
            K.conv1d(st, 4, 16, Y, A=A)
    P = torch.zeros((6, 8), device="cuda")
    for args in (("median", A, P, 4, 16, 8), ("max", A, P.double(), 4, 16, 8), ("max", A, P[:, :4], 4, 16, 8),
                 ("max", A, P, 7, 16, 8), ("max", A, P, 4, 15, 8), ("max", A.cpu(), P, 4, 16, 8), ("max", A, P, 4, 16, 300)):
        with pytest.raises(ValueError):
            K.seq_pool(*args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ end to end
def _ring_store(T):
    """A device store whose event rings hold the GRU edge suite's ring case."""
    import torch
    from tests import gru_cases as G
    from igaming_platform_amd.config import FeatureConfig
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.layouts import ACCTRT
    fc = FeatureConfig()
    ev, head, count, slots = G.ring_case(fc.event_ring, fc.event_dim, T)
    n = ev.shape[0]
    store = DeviceFeatureStore(n, fc, "cuda", events=True, max_events=64)
    store.ev.copy_(torch.from_numpy(ev).to(torch.bfloat16).view(torch.int16).cuda())
    rt = np.zeros(n, ACCTRT)
    rt["ev_head"], rt["ev_count"] = head, count
    store.rt.copy_(torch.from_numpy(rt.view(np.int32).reshape(n, -1).copy()).cuda())
    return store, G.ring_gather(ev, head, count, slots, T), slots


def test_abuse_gpu_with_tcn_plan_matches_direct_run():
    """AbuseGpu (captured graph per bucket: H2D slots -> the conv layers over the event rings -> read-out
    -> head -> D2H) returns what a direct TcnModel.run gives for the same slots, and that is the float64
    reference on the gathered histories within REAL_TOL."""
    import torch
    from igaming_platform_amd.engine.abuse import AbuseGpu
    from igaming_platform_amd.engine.runner import TcnModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    T = 16
    m = C.builders.tcn(seq=T)
    plan = to_device(compile_onnx(native().OnnxModel.from_bytes(m.SerializeToString())), "cuda")
    store, X, slots = _ring_store(T)
    ag = AbuseGpu(store, plan, buckets=(64,), use_graphs=True)
    assert isinstance(ag.gm, TcnModel) and ag.T == T
    ag.capture()
    assert ag.graphs
    got = ag.score_slots(slots)
    tm = TcnModel(plan.steps, "cuda", True, 64)
    out = torch.full((64,), -9.0, device="cuda")
    tm.run(len(slots), T, out, store=store, slots=torch.from_numpy(slots).cuda())
    want = out[:len(slots)].cpu().numpy()
    assert np.all(want != -9.0) and len(set(want.tolist())) > 5
    np.testing.assert_array_equal(got, want)
    err = float(np.abs(want.astype(np.float64) - C.ref_tcn(m, X, seq=T)[:, 0]).max())
    print(f"tcn over the event rings vs float64 on the gathered histories: {err:.3e}")
    assert err <= C.REAL_TOL


def test_risk_engine_gpu_tcn_abuse_model_matches_cpu_backend():
    """builders.tcn as ``abuse_model``: CheckBonusAbuse on backend="gpu" against backend="cpu" (the
    executor over the same encoded events), accounts with 5, 30 and more than 100 events and one
    without any, within REAL_TOL."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.layouts import ACCTBATCH
    now = 1_760_000_000
    m = C.builders.tcn().SerializeToString()
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
    got = np.array([r.model_score for r in rg], np.float64)
    want = np.array([r.model_score for r in rc], np.float64)
    print(f"tcn abuse model gpu vs cpu backend: {got} vs {want}, max diff {np.abs(got - want).max():.3e}")
    assert len(set(np.round(want, 5))) >= 3
    assert np.abs(got - want).max() <= C.REAL_TOL


def test_two_pipeline_slots_back_to_back_equal_direct_runs():
    """A TcnModel keeps one set of activation buffers (``shares_intermediates``), so AbuseGpu keeps its
    pipeline slots on one stream even when asked to overlap them: two different batches submitted
    back to back, before either is waited for, each equal a direct run of their slots."""
    import torch
    from igaming_platform_amd.engine.abuse import AbuseGpu
    from igaming_platform_amd.engine.runner import GruModel, TcnModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    T = 16
    m = C.builders.tcn(seq=T)
    plan = to_device(compile_onnx(native().OnnxModel.from_bytes(m.SerializeToString())), "cuda")
    store, _, slots = _ring_store(T)
    assert TcnModel.shares_intermediates and isinstance(GruModel.shares_intermediates, property)
    ag = AbuseGpu(store, plan, buckets=(64,), use_graphs=True, depth=2, overlap=True)
    assert ag.gm.shares_intermediates and ag.n_streams == 1
    ag.capture()
    a, b = slots[:30].copy(), slots[::-1][:41].copy()
    for _ in range(3):
        pa, pb = ag.submit(a), ag.submit(b)
        got_a, got_b = ag.wait(pa), ag.wait(pb)
        tm = TcnModel(plan.steps, "cuda", True, 64)
        for got, s in ((got_a, a), (got_b, b)):
            out = torch.full((64,), -9.0, device="cuda")
            tm.run(len(s), T, out, store=store, slots=torch.from_numpy(s).cuda())
            np.testing.assert_array_equal(got, out[:len(s)].cpu().numpy())
    assert len(set(got_a.tolist())) > 5


def test_native_abuse_device_keeps_a_tcn_on_one_stream_and_matches_cpu():
    """The native CheckBonusAbuse device (engine/acct.py AbuseNativeDevice, the default GPU path): with a
    TCN its slots share one stream; many requests, micro-batched over both slots, answer as the CPU
    engine's native device does, within REAL_TOL."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.acct import AbuseNativeDevice
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.proto import risk_v1 as P
    from tests.test_acct import _ask, _populate, _requests
    am = C.builders.tcn().SerializeToString()
    cfg = Config()
    cfg.gpu.buckets = [64, 512]
    g = RiskEngine(cfg, backend="gpu", capacity=256, abuse_model=am)
    c = RiskEngine(cfg, backend="cpu", capacity=256, abuse_model=am)
    dev = next(d for d in g.acct.devices if isinstance(d, AbuseNativeDevice))
    assert dev.depth >= 2 and len(dev.streams) == 1
    ids = _populate(g)
    _populate(c)
    reqs = [x for x in _requests(ids) if x[0] == 3] * 3
    a = _ask(g.acct.router, reqs)
    b = _ask(c.acct.router, reqs)
    scores = []
    for (x, ex), (y, ey) in zip(a, b):
        assert ex is None and ey is None
        rx, ry = P.CheckBonusAbuseResponse.FromString(x), P.CheckBonusAbuseResponse.FromString(y)
        assert list(rx.signals) == list(ry.signals) and list(rx.linked_accounts) == list(ry.linked_accounts)
        assert abs(rx.abuse_score - ry.abuse_score) <= C.REAL_TOL, (rx.abuse_score, ry.abuse_score)
        scores.append(rx.abuse_score)
    assert len(set(scores)) > 3
    g.close()
    c.close()
