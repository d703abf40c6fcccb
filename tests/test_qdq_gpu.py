"""QDQ int8 models on the device (csrc/kernels/qgemm.hip): the i8 MFMA lane maps, tails, m_ptr,
requantisation edges, general scales, large sums, quantize_rows / dequantize_rows, DeviceModel on
the ``qdq_mlp`` variants and the engine, against the numpy oracle of tests/quant_cases.py."""
import numpy as np
import pytest

from tests import quant_cases as Q

pytestmark = pytest.mark.gpu

DENSE_TOL = dict(rtol=1e-5, atol=2e-5)   # the suite's fp32 dense tolerance (tests/test_dense_edges_gpu.py)


def _run_layer(c, extra=0, m_ptr=None, m_alloc=None, ldx=None, ldy=None):
    """Launch ``qdense`` on a case: garbage around the live input block, a sentinel-filled output
    with ldy > N (``ldx`` / ``ldy``: strides other than the 16-byte multiples). Returns (Y on the
    host [M_alloc, ldy], ldy)."""
    import torch
    from igaming_platform_amd.models.plan import qdense_tables
    from igaming_platform_amd.ops import kernels as K
    from tests.dense_cases import sentinel_out
    M, N, Kk = c["M"], c["N"], c["K"]
    m_alloc = m_alloc or M + 3
    t = {k: v.cuda() for k, v in qdense_tables(Q.case_step(c)).items()}
    ldx = ldx or -(-Kk // 16) * 16 + extra
    X = Q.garbage_input(m_alloc, ldx, M, Kk, Q.stored(c["xq"], c["x_type"])).cuda()
    if c["out"] is None:
        ldy = ldy or N + 3
        Y = sentinel_out(m_alloc, ldy, torch.float32).cuda()
    else:
        ldy = ldy or -(-N // 16) * 16 + 16
        Y = Q.sentinel_q(m_alloc, ldy).cuda()
    K.qdense(X, t["w8"], t["corr"], t["mult"], t["bias"], Y, M, N, Kk, act=c["act"], out_q=c["out"], m_ptr=m_ptr)
    torch.cuda.synchronize()
    return Y.cpu(), ldy


def _check_layer(c, Y, exact):
    """Compare the live block with the oracle: f32 at the dense tolerance; bytes equal (``exact``),
    else equal off the ambiguous elements and within one quantum on them."""
    from tests.dense_cases import untouched
    M, N = c["M"], c["N"]
    r = Q.case_oracle(c)
    if c["out"] is None:
        assert untouched(Y, M, N)
        np.testing.assert_allclose(Y[:M, :N].numpy(), r["v"], **DENSE_TOL)
        return
    assert Q.untouched_q(Y, M, N)
    got = Q.unstored(Y[:M, :N].numpy(), c["out"][2])
    if exact and c["act"] in ("sigmoid", "tanh"):
        # no f32 sigmoid can promise the byte of a value on a tie: equal off the elements within
        # quant_cases.ACT_TIE_MARGIN quanta of one, within one quantum on them
        near = r["tie"] < Q.ACT_TIE_MARGIN
        assert near.sum() <= 2 + 2e-3 * near.size     # a uniform fraction lands there with probability 4e-4
        np.testing.assert_array_equal(got[~near], r["q"][~near])
        assert np.abs(got - r["q"]).max() <= 1
    elif exact:
        np.testing.assert_array_equal(got, r["q"])
    else:
        amb = r["ambiguous"]
        np.testing.assert_array_equal(got[~amb], r["q"][~amb])
        assert np.abs(got - r["q"]).max() <= 1


# ------------------------------------------------------------------------------ A: lane maps
@pytest.mark.parametrize("M,N,K", [(16, 16, 64), (64, 64, 128)])
def test_lane_maps_exact_integers(M, N, K):
    """mult = 1, bias = 0, f32 out: asymmetric integer patterns in X and W (no symmetry in
    (row, k) or (column, k)) give exactly the int64 product, so every lane feeds the MFMA the k
    bytes of its own row and the C/D map puts each sum in its place."""
    r_, n_, k_ = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    xq = ((r_ * 7 + k_ * 3 + (r_ * k_) % 5) % 23) - 11
    wq = ((n_ * 5 + k_ * 11 + (n_ * n_ + k_) % 7) % 19) - 9
    c = dict(M=M, N=N, K=K, x_type="int8", x_zp=0, xq=xq, wq=wq, w_zp=0, x_scale=np.float32(1.0),
             w_scale=np.ones(N, np.float32), bias=np.zeros(N, np.float32), act="none", out=None)
    Y, _ = _run_layer(c)
    acc = xq.astype(np.int64) @ wq.astype(np.int64).T
    assert np.abs(acc).max() < 2 ** 24 and not np.array_equal(acc, acc.T)
    np.testing.assert_array_equal(Y[:M, :N].numpy().astype(np.int64), acc)


# ------------------------------------------------------------------------------ B: tails
@pytest.mark.parametrize("si", range(len(Q.TAIL_SHAPES)), ids=["M{}-N{}-K{}".format(*s) for s in Q.TAIL_SHAPES])
def test_tails(si):
    """Every shape with uint8 / int8 activations at the zero points of the host-table test, per-tensor
    and per-channel weights, f32 / uint8 / int8 output and act none / relu / sigmoid, at both input
    strides. Power-of-two scales: requantised bytes are equal, f32 at the dense tolerance."""
    from igaming_platform_amd.native import hipk
    M, N, K = Q.TAIL_SHAPES[si]
    assert hipk().qgemm_tile(M, N) == (128 if si == len(Q.TAIL_SHAPES) - 1 else 64)
    assert hipk().qgemm_tile(M - 1, N) == 64 and hipk().qgemm_tile(M, N - 1) == 64
    for j, v in enumerate(Q.tail_variants(si)):
        c = Q.layer_case(M, N, K, pow2=True, seed=100 * si + j, **v)
        for extra in (0, 16):
            Y, _ = _run_layer(c, extra)
            _check_layer(c, Y, exact=True)


@pytest.mark.parametrize("M,N,K", [(65, 17, 65), (33, 130, 257)])
@pytest.mark.parametrize("out", [None, "int8"])
def test_strides_off_the_vector_paths(M, N, K, out):
    """Rows that are no multiple of 16 bytes (ldx = K and K + 3) take the scalar loader, which
    reads the live bytes only; an output stride that is no multiple of 4 stores byte by byte,
    one that is a multiple of 4 but not of 16 stores dwords and the tail bytes."""
    c = Q.layer_case(M, N, K, x_type="uint8", x_zp=3, per_channel=True, out=out, act="relu", pow2=True, seed=M + K)
    for ldx, ldy in ((K, N + 1), (K + 3, N + 2), (K + 3, -(-N // 4) * 4 + 4)):
        Y, _ = _run_layer(c, ldx=ldx, ldy=ldy)
        _check_layer(c, Y, exact=True)


# ------------------------------------------------------------------------------ C: m_ptr
@pytest.mark.parametrize("out", [None, "uint8"])
def test_m_ptr(out):
    import torch
    c = Q.layer_case(130, 65, 129, out=out, act="relu", pow2=True, seed=7)
    for live in (0, 37, 500):
        m = torch.tensor([live], dtype=torch.int32, device="cuda")
        Y, _ = _run_layer(c, m_ptr=m)
        L = min(live, c["M"])
        c2 = dict(c, M=L, xq=c["xq"][:L])
        if L == 0:
            assert (Q.untouched_q(Y, 0, 0) if out else bool((Y == -7.0).all()))
        else:
            _check_layer(c2, Y, exact=True)


# ------------------------------------------------------------------------------ D: requantisation edges
@pytest.mark.parametrize("out", ["uint8", "int8"])
def test_requantisation_edges(out):
    """K = 1, w = 1, s_x = s_w = 1, s_y = 2: v = x + bias runs over exact ties on both sides of
    zero (+-0.5, +-1.5, +-2.5 quanta ...) and far past both ends, at z_y = both extremes of the type."""
    lo, hi = Q.Q_RANGE[out]
    xq = np.arange(-128, 128)[:, None]
    for z_y in (lo, hi):
        for bias in (0.0, 2000.0, -2000.0, 255.0):
            c = dict(M=256, N=3, K=1, x_type="int8", x_zp=0, xq=xq, wq=np.array([[1], [-1], [2]]), w_zp=0,
                     x_scale=np.float32(1.0), w_scale=np.ones(3, np.float32), bias=np.full(3, bias, np.float32),
                     act="none", out=(np.float32(2.0), z_y, out))
            r = Q.case_oracle(c)
            if bias == 0.0:
                assert (r["tie"][:, 0] == 0).sum() == 128          # every odd x is an exact tie
            Y, _ = _run_layer(c)
            _check_layer(c, Y, exact=True)
            if abs(bias) == 2000.0:
                assert len(np.unique(r["q"])) == 1               # saturated at one end


# ------------------------------------------------------------------------------ E: general scales
@pytest.mark.parametrize("seed", Q.GENERAL_SEEDS)
def test_general_scales(seed):
    c = Q.general_case(seed)
    r = Q.case_oracle(c)
    assert r["ambiguous"].mean() <= Q.AMBIGUOUS_CAP     # a condition on the inputs (tests/test_qdq.py checks it too)
    Y, _ = _run_layer(c)
    _check_layer(c, Y, exact=False)


# ------------------------------------------------------------------------------ F: large sums
@pytest.mark.parametrize("out", [None, "uint8", "int8"])
def test_large_sums(out):
    """K = 2048 with every operand at its extreme: x - z_x = -128 (int8 -128, zero point 0) times
    w = -128 -> acc = 2^25 on half the columns, -2^25 + 2^18 (w = 127) on the others."""
    M, N, K = 33, 18, 2048
    wq = np.where(np.arange(N)[:, None] % 2 == 0, -128, 127) * np.ones((1, K), np.int64)
    c = dict(M=M, N=N, K=K, x_type="int8", x_zp=0, xq=np.full((M, K), -128), wq=wq, w_zp=0, x_scale=np.float32(2.0 ** -6),
             w_scale=np.full(N, 2.0 ** -9, np.float32), bias=np.full(N, 0.5, np.float32), act="none",
             out=None if out is None else (np.float32(0.25), 0 if out == "int8" else 128, out))
    r = Q.case_oracle(c)
    assert np.abs(r["acc"]).max() == 2 ** 25
    Y, _ = _run_layer(c)
    _check_layer(c, Y, exact=True)
    if out is not None:
        lo, hi = Q.Q_RANGE[out]
        assert set(np.unique(r["q"])) == {lo, hi}


# ------------------------------------------------------------------------------ G: quantize / dequantize rows
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("qtype,zp", [("uint8", 3), ("int8", -5)])
def test_quantize_dequantize_rows(dtype, qtype, zp):
    import torch
    from igaming_platform_amd.ops import kernels as K
    from tests.dense_cases import sentinel_out, untouched
    dt = getattr(torch, dtype)
    s = np.float32(0.25)
    M = 37
    for N in (1, 15, 17, 130):
        rng = np.random.default_rng(N)
        # quarter-quantum grid: exact in bf16, and every other value an exact tie on both sides of zero
        x = (rng.integers(-1400, 1400, (M, N)) * 0.125).astype(np.float32)
        x.flat[:6] = [0.125, -0.125, 0.375, -0.375, np.inf, -np.inf][:min(6, x.size)]
        ref = Q.quantize64(x, s, zp, qtype)
        for ldx, ldq in ((N, -(-N // 16) * 16), (N + 3, -(-N // 16) * 16 + 16)):
            X = torch.full((M + 2, ldx), float("nan"), dtype=dt)
            X[:M, :N] = torch.from_numpy(x).to(dt)
            for live in (None, 0, 20, 99):
                Y = Q.sentinel_q(M + 2, ldq).cuda()
                m = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
                K.quantize(X.cuda(), Y, M, N, s, zp, qtype, m_ptr=m)
                L = M if live is None else min(live, M)
                Yh = Y.cpu()
                assert Q.untouched_q(Yh, L, N)
                np.testing.assert_array_equal(Q.unstored(Yh[:L, :N].numpy(), qtype), ref[:L])
            # and back: (q - zp) * s is exact in f32 and in bf16 (9-bit integers times 2^-2)
            Qd = Q.garbage_input(M + 2, ldq, M, N, Q.stored(ref, qtype)).cuda()
            F = sentinel_out(M + 2, ldx, dt).cuda()
            m = torch.tensor([20], dtype=torch.int32, device="cuda")
            K.dequantize(Qd, F, M, N, s, zp, qtype, m_ptr=m)
            Fh = F.cpu()
            assert untouched(Fh, 20, N)
            want = Q.dequantize64(ref[:20], s, zp)
            got = Fh[:20, :N].float().numpy()
            if dtype == "float32":
                np.testing.assert_array_equal(got, want)
            else:   # 9-bit integers round to bf16's 8 bits: half an ulp
                np.testing.assert_allclose(got, want, rtol=2.0 ** -8, atol=0)


# ------------------------------------------------------------------------------ H: DeviceModel
def _load(m):
    from igaming_platform_amd.native import native
    return native().OnnxModel.from_bytes(m.SerializeToString())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("widths", Q.MODEL_WIDTHS, ids=["30-64-1", "33-130-17-1"])
@pytest.mark.parametrize("variant", sorted(Q.MODEL_VARIANTS))
def test_device_model_matches_oracle(variant, widths, precision):
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.onnx import builders
    kw, head = Q.MODEL_VARIANTS[variant]
    om = _load(builders.build("qdq_mlp", widths=widths, per_channel=len(widths) > 3, **kw))
    plan = to_device(compile_onnx(om), "cuda", precision=precision)
    kinds = [s.kind for s in plan.steps]
    assert kinds[:len(head)] == head and (kinds[-1] == "dequant") == (variant == "trailing"), plan.describe()
    dm = DeviceModel(plan, "cuda", [64, 300])
    float_layer = variant == "unfused"     # the LeakyRelu row step runs on a float tensor
    n_bad = 0
    for bucket, rows in Q.MODEL_BUCKETS:
        X = Q.model_inputs(bucket, rows, widths[0])
        ref, bad = Q.model_oracle(plan, X)
        Xd = torch.zeros((bucket, widths[0]), dtype=torch.float32, device="cuda")
        Xd[:rows] = torch.from_numpy(X).cuda()
        got = dm.run(Xd, bucket)[:rows].float().cpu().numpy()
        if precision == "bf16" and float_layer:
            np.testing.assert_allclose(got, ref, atol=3e-2, rtol=3e-2)
            continue
        n_bad += int(bad.sum())
        np.testing.assert_allclose(got[~bad], ref[~bad], atol=1e-5, rtol=1e-5)
    assert n_bad <= Q.MODEL_BAD_ROWS * sum(r for _, r in Q.MODEL_BUCKETS), n_bad   # at most 2 % of the rows are left out


def test_tree_with_qdq_head_matches_executor():
    import torch
    from igaming_platform_amd.engine.runner import DeviceModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    om = _load(Q.tree_qdq_model())
    plan = to_device(compile_onnx(om), "cuda")
    assert [s.kind for s in plan.steps] == ["tree", "quant", "qdense"]
    dm = DeviceModel(plan, "cuda", [64])
    X = np.random.default_rng(5).uniform(0, 1, (50, 30)).astype(np.float32)
    res = native().Executor(om).run({"input": X})
    ref, emb = np.asarray(res["output"]), np.asarray(res["emb"], np.float64)
    # the tree kernel sums 16 leaves of |value| ~ 0.1 in another order than the executor: a row with
    # an embedding column that close to a rounding tie of the Q is left out (at most 2 % of rows)
    s = plan.steps[1]
    u = emb / np.float64(s.scale)
    bad = (np.abs(np.abs(u - np.floor(u)) - 0.5) < 64 * Q.EPS * np.maximum(np.abs(emb), 1.0) / np.float64(s.scale)).any(axis=1)
    assert bad.mean() <= 0.02
    Xd = torch.zeros((64, 30), dtype=torch.float32, device="cuda")
    Xd[:50] = torch.from_numpy(X).cuda()
    got = dm.run(Xd, 64)[:50].float().cpu().numpy()
    np.testing.assert_allclose(got[~bad], ref[~bad], atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------ I: engine
@pytest.mark.parametrize("direct", ["1", "0"], ids=["direct", "graph"])
def test_engine_gpu_matches_cpu(direct, monkeypatch):
    """A QDQ fraud model through the GPU scorer (recorded direct launches / graph replay) against
    the CPU backend. Power-of-two scales: every hidden byte is exact on both sides."""
    from igaming_platform_amd.config import Config
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.onnx import builders
    from tests.test_engine_cpu import NOW, _txs
    monkeypatch.setenv("IGP_DIRECT_LAUNCH", direct)
    m = builders.build("qdq_mlp", widths=(30, 64, 1), pow2=True).SerializeToString()
    cfg = Config()
    cfg.gpu.buckets = [64, 256]
    cfg.gpu.max_batch = 256
    g = RiskEngine(cfg, backend="gpu", capacity=512, fraud_model=m)
    c = RiskEngine(cfg, backend="cpu", capacity=512, fraud_model=m)
    txs = _txs(200, np.random.default_rng(12))
    a, b = g.score(txs, now=NOW), c.score(txs, now=NOW)
    np.testing.assert_allclose([x["ml_score"] for x in a], [x["ml_score"] for x in b], atol=1e-5)
    assert np.ptp([x["ml_score"] for x in a]) > 1e-3
    g.close()
    c.close()


def test_gpu_ltv_with_qdq_model_matches_cpu():
    """One PredictLTV batch with a QDQ LTV model (64 inputs): the service runs it step by step
    through DeviceModel and answers as the CPU backend does."""
    from igaming_platform_amd.golden import ltv as GL
    from igaming_platform_amd.onnx import builders
    from tests.test_engine_gpu import _engines
    m = builders.build("qdq_mlp", widths=(64, 64, 1), pow2=True, seed=23).SerializeToString()
    g, c = _engines(ltv_model=m)
    ltv = g.ltv.gpu[0]
    assert ltv.chain is None and [s.kind for s in ltv.plan.steps] == ["quant", "qdense", "qdense"]
    rng = np.random.default_rng(4)
    players = [GL.PlayerFeatures(days_since_registration=int(rng.integers(1, 900)), days_since_last_bet=int(rng.integers(0, 60)),
                                 days_since_last_deposit=int(rng.integers(0, 90)), sessions_per_week=float(rng.uniform(0, 8)),
                                 net_revenue=float(rng.uniform(-500, 30000)), deposit_frequency=float(rng.uniform(0, 6)),
                                 bet_count=int(rng.integers(0, 400)), support_tickets=int(rng.integers(0, 6)))
               for _ in range(100)]
    ids = [f"p{i}" for i in range(100)]
    for e in (g, c):
        e.set_players(ids, players)
    rg, rc = g.predict_ltv_batch(ids), c.predict_ltv_batch(ids)
    for x, y in zip(rg, rc):
        assert x.churn_risk == pytest.approx(y.churn_risk) and x.survival_days == y.survival_days
        assert x.predicted_ltv == pytest.approx(y.predicted_ltv, rel=1e-5, abs=1e-4)
    g.close()
    c.close()
