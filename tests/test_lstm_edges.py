"""The K4 LSTM edge cases of tests/lstm_cases.py without a GPU: the float64 reference against the C++
executor and a hand-computed step, which lstm_kernel instances the case tables reach (through a
mirror of launch_lstm's choice), and the conditions that keep the device test's tolerances honest."""
import numpy as np
import pytest

from tests import lstm_cases as L
from tests.dense_cases import bf16r

# Every instance launch_lstm (lstm.hip) can pick, written out from launch_lstm, launch_lstm_h and
# launch_lstm_t: (RT, KSX, KSH, NW, SPLIT). RT 1 | 2 (tile_rows 16 | 32), KSX 1 | 2 (layer-1 input
# padded to 32 | 64), (KSH, NW) (2, 4) | (4, 8) | (8, 8) at H = 64 | 128 | 256, SPLIT 0 | 1. All 24 fit
# the 160 KiB of LDS; the largest image is <2, 2, 8, 8, 1> at 162816 B.
INSTANCES = [
    (1, 1, 2, 4, 0), (1, 1, 2, 4, 1), (2, 1, 2, 4, 0), (2, 1, 2, 4, 1),
    (1, 2, 2, 4, 0), (1, 2, 2, 4, 1), (2, 2, 2, 4, 0), (2, 2, 2, 4, 1),
    (1, 1, 4, 8, 0), (1, 1, 4, 8, 1), (2, 1, 4, 8, 0), (2, 1, 4, 8, 1),
    (1, 2, 4, 8, 0), (1, 2, 4, 8, 1), (2, 2, 4, 8, 0), (2, 2, 4, 8, 1),
    (1, 1, 8, 8, 0), (1, 1, 8, 8, 1), (2, 1, 8, 8, 0), (2, 1, 8, 8, 1),
    (1, 2, 8, 8, 0), (1, 2, 8, 8, 1), (2, 2, 8, 8, 0), (2, 2, 8, 8, 1),
]


def _run(model_bytes, X):
    from igaming_platform_amd.native import native
    N = native()
    om = N.OnnxModel.from_bytes(model_bytes)
    return np.asarray(N.Executor(om).run({"input": np.ascontiguousarray(X, np.float32)})["output"])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(L.MODELS))
def test_reference_matches_executor(name, reverse):
    """lstm_ref(bf16=False) equals the C++ executor on the ONNX twin (Y_h and the head's output), for
    every model, forward and reverse, on 8 rows at the 2e-6 of test_lstm_gpu.py's _lstm_f64 check."""
    m = L.MODELS[name]
    X = L.dense_x(name)[:, :8]
    layers, head = L.weights(name)
    yh, out = L.lstm_ref(layers, head, X, reverse=reverse)
    got_h = _run(L.onnx_lstm(name, m.T, reverse, head=False), X).reshape(8, m.H)
    got_o = _run(L.onnx_lstm(name, m.T, reverse, head=True), X).reshape(-1)
    np.testing.assert_allclose(got_h, yh, rtol=0, atol=L.EXECUTOR_TOL)
    np.testing.assert_allclose(got_o, out, rtol=0, atol=L.EXECUTOR_TOL)


@pytest.mark.parametrize("name", list(L.BI_MODELS))
def test_bidirectional_reference_matches_executor(name):
    """bi_ref (forward | reverse final states in the ONNX [N, 2, H] order, the head over 2H) equals the
    executor on the bidirectional twin."""
    m = L.BI_MODELS[name]
    X = L.dense_x(name)[:, :8]
    yh, out = L.bi_ref(name, X)
    np.testing.assert_allclose(_run(L.onnx_bilstm(name, head=False), X).reshape(8, 2 * m.H), yh, rtol=0,
                               atol=L.EXECUTOR_TOL)
    np.testing.assert_allclose(_run(L.onnx_bilstm(name, head=True), X).reshape(-1), out, rtol=0, atol=L.EXECUTOR_TOL)


def test_hand_computed_step():
    """A 1-unit, 1-input LSTM with numbers worked out here: gate order i, o, f, c (every gate has its
    own weight, so a swapped pair changes the result), f on the old cell state and i on the candidate,
    Wb + Rb; then the bf16 rounding points on two steps of A's layer."""
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    # rows of W / R / the bias halves: i, o, f, c; all values exact in bf16
    W = np.array([[0.5], [-1.0], [2.0], [0.25]], np.float32)
    R = np.array([[1.0], [0.5], [-0.5], [2.0]], np.float32)
    B = np.array([0.5, 0.25, -0.5, 1.0, 0.5, -0.25, 0.25, -0.5], np.float32)  # Wb | Rb
    x = np.array([[[2.0]], [[-1.0]]], np.float32)
    # step 1 (h0 = c0 = 0, so f has no say): pre-activations W x + Wb + Rb
    i1, o1, g1 = sig(0.5 * 2 + 1.0), sig(-1.0 * 2 + 0.0), np.tanh(0.25 * 2 + 0.5)
    c1 = i1 * g1
    h1 = o1 * np.tanh(c1)
    assert abs(c1 - 0.880797 * 0.761594) < 1e-6 and abs(h1 - 0.119203 * np.tanh(0.670810)) < 1e-6
    yh, _ = L.lstm_ref([(W, R, B)], None, x[:1])
    np.testing.assert_allclose(yh, [[h1]], rtol=0, atol=1e-15)
    # step 2: x = -1, the recurrent product on h1, f on c1
    i2 = sig(0.5 * -1 + 1.0 * h1 + 1.0)
    o2 = sig(-1.0 * -1 + 0.5 * h1 + 0.0)
    f2 = sig(2.0 * -1 - 0.5 * h1 - 0.25)
    g2 = np.tanh(0.25 * -1 + 2.0 * h1 + 0.5)
    c2 = f2 * c1 + i2 * g2
    h2 = o2 * np.tanh(c2)
    yh, out = L.lstm_ref([(W, R, B)], (np.array([3.0], np.float32), 0.125, "sigmoid"), x)
    np.testing.assert_allclose(yh, [[h2]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out, [sig(3.0 * h2 + 0.125)], rtol=0, atol=1e-15)
    # any two gates swapped give another h2: the check above pins the order
    for a in range(4):
        for b in range(a + 1, 4):
            p = list(range(4))
            p[a], p[b] = b, a
            sw, _ = L.lstm_ref([(W[p], R[p], np.concatenate([B[:4][p], B[4:][p]]))], None, x)
            assert abs(sw[0, 0] - h2) > 1e-3, (a, b)
    # reverse reads the sequence last step first
    ra = L.lstm_ref([(W, R, B)], None, x, reverse=True)[0]
    np.testing.assert_array_equal(ra, L.lstm_ref([(W, R, B)], None, x[::-1])[0])
    assert abs(ra[0, 0] - h2) > 1e-3

    # the bf16 rounding points, on A's layer and one row: x (ties to even), W, R and the h operand of
    # the next step's recurrent product round; c and the h that reaches yh and the head do not
    (Wa, Ra, Ba), = L.weights("A")[0]
    H, head = 64, L.weights("A")[1]
    xa = np.array([[[1.0 + 2.0 ** -8, -0.3, 0.7, 1.0 + 3 * 2.0 ** -8, 0.1, -2.0, 0.55, 0.25]],
                   [[0.5, 1.3, -0.7, 0.2, -1.1, 0.9, 0.33, -0.05]]], np.float32)
    assert bf16r(xa[0, 0, [0, 3]]).tolist() == [1.0, 1.0 + 2.0 ** -6]
    Wq, Rq = bf16r(Wa), bf16r(Ra)
    bias = (Ba[:4 * H] + Ba[4 * H:]).astype(np.float64)
    assert bias.dtype == np.float64 and (Ba[:4 * H] + Ba[4 * H:]).dtype == np.float32
    gates = lambda a: (sig(a[:H]), sig(a[H:2 * H]), sig(a[2 * H:3 * H]), np.tanh(a[3 * H:]))
    i, o, f, g = gates(Wq @ bf16r(xa[0, 0]) + bias)
    c1 = i * g
    h1 = o * np.tanh(c1)
    yh, out = L.lstm_ref([(Wa, Ra, Ba)], head, xa[:1], bf16=True)
    np.testing.assert_allclose(yh[0], h1, rtol=0, atol=1e-15)
    np.testing.assert_allclose(out[0], sig(h1 @ head[0].astype(np.float64) + head[1]), rtol=0, atol=1e-15)
    hq = bf16r(h1)
    assert np.any(hq != h1)
    i, o, f, g = gates(Wq @ bf16r(xa[1, 0]) + Rq @ hq + bias)
    h2 = o * np.tanh(f * c1 + i * g)
    yh, _ = L.lstm_ref([(Wa, Ra, Ba)], None, xa, bf16=True)
    np.testing.assert_allclose(yh[0], h2, rtol=0, atol=1e-15)
    # a second layer reads the rounded h of the first
    (W2, R2, B2) = L.weights("B")[0][1]
    b2 = (B2[:4 * H] + B2[4 * H:]).astype(np.float64)
    i, o, f, g = gates(bf16r(W2) @ hq + b2)
    yh, _ = L.lstm_ref([(Wa, Ra, Ba), (W2, R2, B2)], None, xa[:1], bf16=True)
    np.testing.assert_allclose(yh[0], o * np.tanh(i * g), rtol=0, atol=1e-15)


def test_ring_gather():
    """Right-aligned, oldest first, the last T entries before ev_head, min(ev_count, T) live: counts
    0, 3, T and more than T (wrapped), slot -1; in reverse the reference walks it last step first."""
    ev = np.arange(3 * 5 * 1, dtype=np.float32).reshape(3, 5, 1) + 1
    X = L.ring_gather(ev, np.array([1, 4, 2]), np.array([2, 5, 0]), np.array([0, -1, 1, 2, 0]), 3)
    assert X[:, 0, 0].tolist() == [0.0, 5.0, 1.0]     # head 1, count 2: entries 4, 0 are the newest two
    assert X[:, 1, 0].tolist() == [0.0, 0.0, 0.0]     # slot -1
    assert X[:, 2, 0].tolist() == [7.0, 8.0, 9.0]     # head 4, count 5 > T: entries 1, 2, 3
    assert X[:, 3, 0].tolist() == [0.0, 0.0, 0.0]     # count 0
    assert X[:, 4, 0].tolist() == X[:, 0, 0].tolist()  # a repeated slot
    X = L.ring_gather(ev, np.array([1, 1, 1]), np.array([3, 5, 5]), np.array([0, 1]), 3)
    assert X[:, 0, 0].tolist() == [4.0, 5.0, 1.0]     # count = T, wrapped round the ring's end
    assert X[:, 1, 0].tolist() == [9.0, 10.0, 6.0]
    from igaming_platform_amd.config import FeatureConfig
    assert FeatureConfig().event_dim == L.MODELS["E"].I == 16
    for T in L.RING_T:
        ev, head, count, slots = L.ring_case(T)
        live = slots[slots >= 0]
        assert ev.shape[1] == L.RING >= T and len(slots) == L.RING_ROWS
        assert {0, 3, T, L.RING} <= set(count[live].tolist())
        assert any(count[s] >= T and head[s] < T for s in live)            # wrapped
        assert (slots < 0).sum() >= 2 and len(set(live.tolist())) < len(live)  # slot -1 and repeats
        assert len(L.ring_empty_rows(T)) >= 4
        np.testing.assert_array_equal(bf16r(ev), ev)  # x is exact in bf16
        X = L.ring_x(T)
        assert not X[:, L.ring_empty_rows(T)].any()
        layers, hd = L.weights("E")
        a = L.lstm_ref(layers, hd, X, reverse=True, bf16=True)
        b = L.lstm_ref(layers, hd, X[::-1], bf16=True)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[0], L.reference(f"E-ring-{T}-reverse", True)[0])


def test_case_tables_cover_every_instance():
    """The tables reach all 24 instances of lstm_kernel; T = 1, 2, 3 at H = 256; 1 to 8 staging chunks
    per row; reverse, the event rings and a live count that leaves one row in the last workgroup at
    either tile size."""
    assert len(INSTANCES) == len(set(INSTANCES)) == 24
    reached = {inst for n in L.MODELS for split in (False, True) for _, inst in L.paths(n, split)}
    assert reached == set(INSTANCES)
    for n in L.MODELS:
        for split in (False, True):
            p = L.paths(n, split)
            assert [o["tile_rows"] for o, _ in p] == [16, 32] and p[0][1][0] == 1 and p[1][1][0] == 2
            assert p[0][1] == L.dispatch(L.MODELS[n], 0, split) == L.dispatch(L.MODELS[n], 16, split)
    # the dispatch mirror's LDS formula: the figures of lstm.hip / the issue, all within the limit
    assert L.lds_bytes(2, 2, 8, 8, 1) == 162816 == max(L.lds_bytes(*i) for i in INSTANCES) <= L.LDS_LIMIT == 163840
    # all six (H, KSX) pairs, both layer counts at each H
    assert {(m.H, 1 if m.I <= 32 else 2) for m in L.MODELS.values()} == {(h, k) for h in (64, 128, 256) for k in (1, 2)}
    assert {(m.H, m.layers) for m in L.MODELS.values()} == {(h, n) for h in (64, 128, 256) for n in (1, 2)}
    assert {m.T for m in L.MODELS.values() if m.H == 256} >= {1, 2, 3}
    assert {m.I // 8 for m in L.MODELS.values()} == set(range(1, 9))
    for v in ("E_T1", "E_T2", "E_T3"):  # E's weights
        for a, b in zip(L.weights(v)[0], L.weights("E")[0]):
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert L.MODELS["A_none"].act == "none" and np.array_equal(L.weights("A_none")[1][0], L.weights("A")[1][0])
    assert all(m.act == "sigmoid" for n, m in L.MODELS.items() if n != "A_none")
    assert all(L.weights(n)[1][1] == 0.125 for n in L.MODELS)
    assert L.REVERSE_MODELS == ["B", "E"] and L.RING_T == [7, L.RING]
    labels = {lab for lab, *_ in L.ref_inputs()}
    assert {"B-dense-reverse", "E-dense-reverse", "E-ring-7", "E-ring-7-reverse", f"E-ring-{L.RING}",
            f"E-ring-{L.RING}-reverse"} <= labels
    assert L.BP_LIVE == [(47, None), (47, 33), (47, 16), (47, 0), (1, None)]
    assert 33 % 16 == 33 % 32 == 1 and L.BP_XROWS == 50 > L.BP_ROWS
    assert max([r for r, _ in L.BP_LIVE] + [L.RING_ROWS, L.BP_XROWS] + L.BI_ROWS) <= 64
    assert max(m.T for m in L.MODELS.values()) <= 12 and L.RING <= 12
    assert {(m.H, m.I) for m in L.BI_MODELS.values()} == {(64, 40), (256, 16)} and L.BI_ROWS == [1, 47]


def test_tolerances_come_from_the_reference():
    """Conditions (a) - (d) of the K4 LSTM edge tests.
    (a) the bf16 emulation in float32 against the same in float64 stays within TOL / 4 on every
        reference input, and the tolerances are no wider than 4x the measured maximum (+ 5 %);
    (b) a dropped hidden unit (at the median |head weight|), the last layer's Rb ignored and the last
        input column ignored each move yh or out by at least 4x its tolerance on every model, and the
        device test's comparison rejects them;
    (c) the reference scores of every model span at least 0.25 between the 5th and 95th percentile;
    (d) the comparison takes every live row (it has no skip list: see lstm_cases.compare)."""
    mx = {"yh": 0.0, "sigmoid": 0.0, "none": 0.0}
    for label, name, X, rev in L.ref_inputs():
        layers, head = L.weights(name)
        yh_tol, out_tol = L.tol(name)
        yh, out = L.reference(label, True)
        yh32, out32 = L.lstm_ref(layers, head, X, reverse=rev, bf16=True, dtype=np.float32)
        assert yh32.dtype == out32.dtype == np.float32
        gy, go = float(np.abs(yh32 - yh).max()), float(np.abs(out32 - out).max())
        print(f"{label}: f32 emulation off by yh {gy:.2e} out {go:.2e}")
        assert gy <= yh_tol / 4 and go <= out_tol / 4, (label, gy, go)                # (a)
        mx["yh"], mx[head[2]] = max(mx["yh"], gy), max(mx[head[2]], go)
        lo, hi = np.percentile(out, [5, 95])
        assert hi - lo >= 0.25, (label, hi - lo)                                      # (c)
        if not label.endswith("-dense"):
            continue
        rows = X.shape[1]
        for probe in L.probes(name):                                                  # (b)
            pyh, pout = L.lstm_ref(layers, head, X, reverse=rev, bf16=True, probe=probe)
            dy, do = float(np.abs(pyh - yh).max()), float(np.abs(pout - out).max())
            assert dy >= 4 * yh_tol or do >= 4 * out_tol, (label, probe, dy, do)
            with pytest.raises(AssertionError, match="off by"):
                L.compare(pyh.astype(np.float32), pout.astype(np.float32), yh, out, rows, yh_tol, out_tol)
    print("measured maxima:", mx)
    assert L.YH_TOL <= 4 * mx["yh"] * 1.05 and L.OUT_TOL <= 4 * mx["sigmoid"] * 1.05, mx
    assert L.LOGIT_TOL <= 4 * mx["none"] * 1.05, mx
    assert L.SPLIT_TOL == 1e-4 and L.EXECUTOR_TOL == 2e-6


def test_compare_checks_every_row():
    """(d): one row off, a NaN, or a write past the live rows fails the comparison, wherever it is;
    a live count of 0 means nothing may be written."""
    yh, out = L.reference("A-dense", True)
    rows, live = 50, 47
    bads = (None, ("yh", 46, 2 * L.YH_TOL), ("yh", 0, -2 * L.YH_TOL), ("out", 0, 2 * L.OUT_TOL),
            ("out", 46, -2 * L.OUT_TOL), ("yh", 13, np.nan), ("out", 20, np.nan), ("yh", 47, 0.5), ("out", 49, 0.0))
    for bad in bads:
        gy = np.full((rows, 64), L.SENTINEL, np.float32)
        go = np.full(rows, L.SENTINEL, np.float32)
        gy[:live], go[:live] = yh[:live], out[:live]
        if bad is None:
            L.compare(gy, go, yh, out, live, L.YH_TOL, L.OUT_TOL)
            continue
        arr, row, d = bad
        if arr == "yh":
            gy[row, 63] = gy[row, 63] + d if row < live else d
        else:
            go[row] = go[row] + d if row < live else d
        with pytest.raises(AssertionError):
            L.compare(gy, go, yh, out, live, L.YH_TOL, L.OUT_TOL)
    gy = np.full((rows, 64), L.SENTINEL, np.float32)
    go = np.full(rows, L.SENTINEL, np.float32)
    assert L.compare(gy, go, yh, out, 0, L.YH_TOL, L.OUT_TOL) == (0.0, 0.0)
    go[0] = out[0]
    with pytest.raises(AssertionError, match="past the live rows"):
        L.compare(gy, go, yh, out, 0, L.YH_TOL, L.OUT_TOL)
