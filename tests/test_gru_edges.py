"""The K4 edge cases of tests/gru_cases.py without a GPU: the float64 reference against the C++
executor and a hand-computed step, which kernel instances the case tables reach (through a mirror of
launch_gru's choice), and the conditions that keep the device test's tolerances honest."""
import numpy as np
import pytest

from tests import gru_cases as G
from tests.dense_cases import bf16r

# Every instance launch_gru (gru.hip) can pick for H in {64, 128, 256}, written out from launch_gru,
# launch_gru_t and launch_gru_x3: (kernel, RT, KSX, KSH, LBR, NW).
# gru_kernel: RT 1 | 2 (tile_rows), KSX 1 | 2 (input K padding 32 | 64), 4 waves at H = 64, 8 or
# (waves = 4) 4 at H >= 128, both linear_before_reset forms.
GRU_KERNEL = [
    ("gru_kernel", 1, 1, 2, 0, 4), ("gru_kernel", 1, 1, 2, 1, 4),
    ("gru_kernel", 1, 2, 2, 0, 4), ("gru_kernel", 1, 2, 2, 1, 4),
    ("gru_kernel", 2, 1, 2, 0, 4), ("gru_kernel", 2, 1, 2, 1, 4),
    ("gru_kernel", 2, 2, 2, 0, 4), ("gru_kernel", 2, 2, 2, 1, 4),
    ("gru_kernel", 1, 1, 4, 0, 4), ("gru_kernel", 1, 1, 4, 1, 4),
    ("gru_kernel", 1, 2, 4, 0, 4), ("gru_kernel", 1, 2, 4, 1, 4),
    ("gru_kernel", 2, 1, 4, 0, 4), ("gru_kernel", 2, 1, 4, 1, 4),
    ("gru_kernel", 2, 2, 4, 0, 4), ("gru_kernel", 2, 2, 4, 1, 4),
    ("gru_kernel", 1, 1, 4, 0, 8), ("gru_kernel", 1, 1, 4, 1, 8),
    ("gru_kernel", 1, 2, 4, 0, 8), ("gru_kernel", 1, 2, 4, 1, 8),
    ("gru_kernel", 2, 1, 4, 0, 8), ("gru_kernel", 2, 1, 4, 1, 8),
    ("gru_kernel", 2, 2, 4, 0, 8), ("gru_kernel", 2, 2, 4, 1, 8),
    ("gru_kernel", 1, 1, 8, 0, 4), ("gru_kernel", 1, 1, 8, 1, 4),
    ("gru_kernel", 1, 2, 8, 0, 4), ("gru_kernel", 1, 2, 8, 1, 4),
    ("gru_kernel", 2, 1, 8, 0, 4), ("gru_kernel", 2, 1, 8, 1, 4),
    ("gru_kernel", 2, 2, 8, 0, 4), ("gru_kernel", 2, 2, 8, 1, 4),
    ("gru_kernel", 1, 1, 8, 0, 8), ("gru_kernel", 1, 1, 8, 1, 8),
    ("gru_kernel", 1, 2, 8, 0, 8), ("gru_kernel", 1, 2, 8, 1, 8),
    ("gru_kernel", 2, 1, 8, 0, 8), ("gru_kernel", 2, 1, 8, 1, 8),
    ("gru_kernel", 2, 2, 8, 0, 8), ("gru_kernel", 2, 2, 8, 1, 8),
]
# gru2_pipe_kernel: H / 32 waves per layer -> NW = 4 / 8 / 16 at H = 64 / 128 / 256
GRU2_PIPE = [
    ("gru2_pipe_kernel", 1, 1, 2, 0, 4), ("gru2_pipe_kernel", 1, 1, 2, 1, 4), ("gru2_pipe_kernel", 1, 2, 2, 0, 4),
    ("gru2_pipe_kernel", 1, 2, 2, 1, 4), ("gru2_pipe_kernel", 2, 1, 2, 0, 4), ("gru2_pipe_kernel", 2, 1, 2, 1, 4),
    ("gru2_pipe_kernel", 2, 2, 2, 0, 4), ("gru2_pipe_kernel", 2, 2, 2, 1, 4),
    ("gru2_pipe_kernel", 1, 1, 4, 0, 8), ("gru2_pipe_kernel", 1, 1, 4, 1, 8), ("gru2_pipe_kernel", 1, 2, 4, 0, 8),
    ("gru2_pipe_kernel", 1, 2, 4, 1, 8), ("gru2_pipe_kernel", 2, 1, 4, 0, 8), ("gru2_pipe_kernel", 2, 1, 4, 1, 8),
    ("gru2_pipe_kernel", 2, 2, 4, 0, 8), ("gru2_pipe_kernel", 2, 2, 4, 1, 8),
    ("gru2_pipe_kernel", 1, 1, 8, 0, 16), ("gru2_pipe_kernel", 1, 1, 8, 1, 16), ("gru2_pipe_kernel", 1, 2, 8, 0, 16),
    ("gru2_pipe_kernel", 1, 2, 8, 1, 16), ("gru2_pipe_kernel", 2, 1, 8, 0, 16), ("gru2_pipe_kernel", 2, 1, 8, 1, 16),
    ("gru2_pipe_kernel", 2, 2, 8, 0, 16), ("gru2_pipe_kernel", 2, 2, 8, 1, 16),
]
# gru_x3_kernel: 32-row tiles only with linear_before_reset; at H = 256 16 waves unless waves = 8 or
# lbr = 0, and no 32-row tile at KSX = 2 (its LDS image, 167936 B / 166912 B at 16 / 8 waves, is over
# the 160 KB: launch_gru_x3 then runs the 16-row kernel of 8 waves)
GRU_X3 = [
    ("gru_x3_kernel", 1, 1, 2, 0, 4), ("gru_x3_kernel", 1, 1, 2, 1, 4), ("gru_x3_kernel", 2, 1, 2, 1, 4),
    ("gru_x3_kernel", 1, 2, 2, 0, 4), ("gru_x3_kernel", 1, 2, 2, 1, 4), ("gru_x3_kernel", 2, 2, 2, 1, 4),
    ("gru_x3_kernel", 1, 1, 4, 0, 8), ("gru_x3_kernel", 1, 1, 4, 1, 8), ("gru_x3_kernel", 2, 1, 4, 1, 8),
    ("gru_x3_kernel", 1, 2, 4, 0, 8), ("gru_x3_kernel", 1, 2, 4, 1, 8), ("gru_x3_kernel", 2, 2, 4, 1, 8),
    ("gru_x3_kernel", 1, 1, 8, 0, 8), ("gru_x3_kernel", 1, 1, 8, 1, 8), ("gru_x3_kernel", 2, 1, 8, 1, 8),
    ("gru_x3_kernel", 1, 1, 8, 1, 16), ("gru_x3_kernel", 2, 1, 8, 1, 16),
    ("gru_x3_kernel", 1, 2, 8, 0, 8), ("gru_x3_kernel", 1, 2, 8, 1, 8), ("gru_x3_kernel", 1, 2, 8, 1, 16),
]
CLUSTER = [("gru_ws_kernel<false>",), ("gru_ws_kernel<true>",), ("gru_ws2_kernel",), ("gru_wsx_kernel",)]


def _run(model_bytes, X):
    from igaming_platform_amd.native import native
    N = native()
    om = N.OnnxModel.from_bytes(model_bytes)
    return np.asarray(N.Executor(om).run({"input": np.ascontiguousarray(X, np.float32)})["output"])


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(G.MODELS))
def test_reference_matches_executor(name, reverse):
    """gru_ref(bf16=False) equals the C++ executor on the ONNX twin (Y_h and the head's output), for
    every model, forward and reverse, at the 2e-6 of test_gru_gpu.py's _gru_f64 check."""
    m = G.MODELS[name]
    X = G.dense_x(name)[:, :G.BP_ROWS]
    layers, head = G.weights(name)
    yh, out = G.gru_ref(layers, head, X, reverse=reverse)
    got_h = _run(G.onnx_gru(name, m.T, reverse, head=False), X).reshape(G.BP_ROWS, m.H)
    got_o = _run(G.onnx_gru(name, m.T, reverse, head=True), X).reshape(-1)
    np.testing.assert_allclose(got_h, yh, rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_o, out, rtol=0, atol=2e-6)


def test_hand_computed_steps():
    """Two steps of A's layer on one row, worked by hand: gate order z, r, h; Wb + Rb; the reset gate
    on (R_h h + Rb_h) (linear_before_reset = 1); x, W, R and the h operand of the recurrent product
    rounded to bf16, the carried state not; and the same weights in the lbr = 0 form, with r * h rounded."""
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    (W, R, B, lbr), = G.weights("A")[0]
    H, head = 64, G.weights("A")[1]
    assert lbr == 1
    x = np.array([[[1.0 + 2.0 ** -8, -0.3, 0.7, 1.0 + 3 * 2.0 ** -8, 0.1, -2.0, 0.55, 0.25]],
                  [[0.5, 1.3, -0.7, 0.2, -1.1, 0.9, 0.33, -0.05]]], np.float32)
    assert bf16r(x[0, 0, [0, 3]]).tolist() == [1.0, 1.0 + 2.0 ** -6]  # ties to even
    v = np.random.default_rng(0).standard_normal(4096) * 10.0 ** np.random.default_rng(1).integers(-6, 6, 4096)
    np.testing.assert_array_equal(G.bf16_rne(np.concatenate([v, x.reshape(-1), [0.0, -0.0]])),
                                  bf16r(np.concatenate([v, x.reshape(-1), [0.0, -0.0]])))
    Wq, Rq, B = bf16r(W), bf16r(R), B.astype(np.float64)
    Wz, Wr, Wh = Wq[:H], Wq[H:2 * H], Wq[2 * H:]
    Rz, Rr, Rh = Rq[:H], Rq[H:2 * H], Rq[2 * H:]
    Wbz, Wbr, Wbh, Rbz, Rbr, Rbh = (B[i * H:(i + 1) * H] for i in range(6))
    x0, x1 = bf16r(x[0, 0]), bf16r(x[1, 0])
    z = sig(Wz @ x0 + Wbz + Rbz)
    r = sig(Wr @ x0 + Wbr + Rbr)
    h1 = (1 - z) * np.tanh(Wh @ x0 + Wbh + r * Rbh)          # h_0 = 0
    yh, out = G.gru_ref([(W, R, B, 1)], head, x[:1], bf16=True)
    np.testing.assert_allclose(yh[0], h1, rtol=0, atol=1e-15)
    np.testing.assert_allclose(out[0], sig(h1 @ head[0].astype(np.float64) + head[1]), rtol=0, atol=1e-15)
    hq = bf16r(h1)
    assert np.any(hq != h1)
    z = sig(Wz @ x1 + Rz @ hq + Wbz + Rbz)
    r = sig(Wr @ x1 + Rr @ hq + Wbr + Rbr)
    h2 = (1 - z) * np.tanh(Wh @ x1 + Wbh + r * (Rh @ hq + Rbh)) + z * h1
    yh, _ = G.gru_ref([(W, R, B, 1)], None, x, bf16=True)
    np.testing.assert_allclose(yh[0], h2, rtol=0, atol=1e-15)
    # linear_before_reset = 0: Rh multiplies bf16(r * h) with the unrounded h, Rb_h outside
    h1 = (1 - sig(Wz @ x0 + Wbz + Rbz)) * np.tanh(Wh @ x0 + Wbh + Rbh)
    hq = bf16r(h1)
    z = sig(Wz @ x1 + Rz @ hq + Wbz + Rbz)
    r = sig(Wr @ x1 + Rr @ hq + Wbr + Rbr)
    assert np.any(bf16r(r * h1) != bf16r(r * hq))
    h2 = (1 - z) * np.tanh(Wh @ x1 + Wbh + Rh @ bf16r(r * h1) + Rbh) + z * h1
    yh, _ = G.gru_ref([(W, R, B, 0)], None, x, bf16=True)
    np.testing.assert_allclose(yh[0], h2, rtol=0, atol=1e-15)
    # reverse reads the sequence last step first
    a = G.gru_ref([(W, R, B, 1)], head, x, reverse=True, bf16=True)
    b = G.gru_ref([(W, R, B, 1)], head, x[::-1], bf16=True)
    np.testing.assert_array_equal(a[0], b[0])


def test_ring_gather():
    """Right-aligned, oldest first, the last T entries before ev_head, min(ev_count, T) live."""
    ev = np.arange(2 * 5 * 1, dtype=np.float32).reshape(2, 5, 1) + 1
    X = G.ring_gather(ev, np.array([1, 4]), np.array([2, 5]), np.array([0, -1, 1]), 3)
    assert X[:, 0, 0].tolist() == [0.0, 5.0, 1.0]     # head 1: entries 4, 0 are the newest two
    assert X[:, 1, 0].tolist() == [0.0, 0.0, 0.0]
    assert X[:, 2, 0].tolist() == [7.0, 8.0, 9.0]     # head 4, count 5 > T: entries 1, 2, 3
    ring, D = G.default_ring()
    assert D == G.MODELS["E"].I and ring > 7
    for T in G.RING_T:
        Tn = ring if T == "ring" else T
        ev, head, count, slots = G.ring_case(ring, D, Tn)
        assert {0, 1, Tn - 1, Tn, ring} <= set(count[slots[slots >= 0]].tolist())
        assert Tn == ring or Tn + 1 in count[slots[slots >= 0]]
        assert {0, 1, ring - 1} <= set(head[slots[slots >= 0]].tolist()) and (slots < 0).sum() >= 2
        np.testing.assert_array_equal(bf16r(ev), ev)  # x is exact in bf16


def test_case_tables_cover_every_instance():
    """The tables reach every instance of the three batch-parallel kernels and the four cluster
    kernels; T = 1, 2, 3 on the pipelined and on every cluster kernel; both input modes and reverse
    on each kernel family."""
    bf = {inst for n in G.MODELS for _, inst in G.bf16_paths(n)}
    x3 = {inst for n in G.MODELS for _, inst in G.split_paths(n)}
    assert bf == set(GRU_KERNEL) | set(GRU2_PIPE)
    assert x3 == set(GRU_X3)
    assert len(set(GRU_KERNEL)) == 40 and len(set(GRU2_PIPE)) == 24 and len(set(GRU_X3)) == 20
    for n in G.MODELS:  # the anchor is the default path: what launch_gru picks with no option set
        assert G.bf16_paths(n)[0][1] == G.dispatch(G.MODELS[n], rows=G.BP_ROWS)
    cl = set()
    for n in G.CLUSTER_MODELS:
        m = G.MODELS[n]
        for ws, rows in G.CLUSTER_ROWS.items():
            for r, _ in rows:
                inst = G.dispatch(m, rows=r, ws=3 if ws == "wsx" else ws, split=ws == "wsx")
                assert inst == (G.CLUSTER_KERNEL[ws],)
                cl.add(inst)
    assert cl == set(CLUSTER)
    assert {G.MODELS[n].T for n in G.CLUSTER_MODELS} >= {1, 2, 3}
    pipe_T = {G.MODELS[n].T for n in G.MODELS if G.bf16_paths(n)[0][1][0] == "gru2_pipe_kernel"}
    assert pipe_T >= {1, 2, 3}
    # reverse and the event rings run on E (every bf16 / split instance of it and the four cluster
    # kernels), reverse also on B: gru_kernel, gru2_pipe_kernel, gru_x3_kernel and the cluster kernels
    assert set(G.REVERSE_MODELS) == {"B", "E"}
    fam = {inst[0] for n in ("E",) for _, inst in G.bf16_paths(n) + G.split_paths(n)}
    assert fam == {"gru_kernel", "gru2_pipe_kernel", "gru_x3_kernel"} and "E" in G.CLUSTER_MODELS
    # live counts: one live row in the last workgroup at either tile size, whole workgroups without
    assert (47, 33) in G.BP_LIVE and 33 % 16 == 1 and 33 % 32 == 1 and (47, 16) in G.BP_LIVE
    assert G.BP_XROWS > G.BP_ROWS
    for ws, rows in G.CLUSTER_ROWS.items():
        per = {1: 128, 2: 128, 3: 64, "wsx": 32}[ws]
        assert {1, per - 1, per + 1} <= {r for r, _ in rows}
        assert any(live is not None and live % per for _, live in rows)
        assert max(r for r, _ in rows) <= 160


def test_tolerances_come_from_the_reference():
    """Conditions (a) - (d) of the K4 edge tests.
    (a) the bf16 emulation in float32 against the same in float64 stays within TOL / 4 on every
        reference input, and the tolerances are no wider than 4x the measured maximum (+ 5 %);
    (b) a dropped hidden unit, a zeroed Rb_h bias and an ignored input column each move yh or out by
        at least 4x its tolerance on every model, and the device test's comparison rejects them;
    (c) the reference scores of every model span at least 0.25 between the 5th and 95th percentile;
    (d) the comparison takes every live row (it has no skip list: see gru_cases.compare)."""
    my = mo = 0.0
    for label, name, X, rev in G.ref_inputs():
        layers, head = G.weights(name)
        yh, out = G.reference(label, True)
        yh32, out32 = G.gru_ref(layers, head, X, reverse=rev, bf16=True, dtype=np.float32)
        gy, go = float(np.abs(yh32 - yh).max()), float(np.abs(out32 - out).max())
        assert gy <= G.YH_TOL / 4 and go <= G.OUT_TOL / 4, (label, gy, go)          # (a)
        my, mo = max(my, gy), max(mo, go)
        lo, hi = np.percentile(out, [5, 95])
        assert hi - lo >= 0.25, (label, hi - lo)                                    # (c)
        if not label.endswith("-dense"):
            continue
        rows = X.shape[1]
        for probe in G.probes(name):                                                # (b)
            pyh, pout = G.gru_ref(layers, head, X, reverse=rev, bf16=True, probe=probe)
            dy, do = float(np.abs(pyh - yh).max()), float(np.abs(pout - out).max())
            assert dy >= 4 * G.YH_TOL or do >= 4 * G.OUT_TOL, (label, probe, dy, do)
            with pytest.raises(AssertionError, match="off by"):
                G.compare(pyh.astype(np.float32), pout.astype(np.float32), yh, out, rows, G.YH_TOL, G.OUT_TOL)
    assert G.YH_TOL <= 4 * my * 1.05 and G.OUT_TOL <= 4 * mo * 1.05, (my, mo)


def test_compare_checks_every_row():
    """(d): one row off, a NaN, or a write past the live rows fails the comparison, wherever it is."""
    yh, out = G.reference("A-dense", True)
    rows, live = 50, 47
    bads = (None, ("yh", 46, 2 * G.YH_TOL), ("out", 0, 2 * G.OUT_TOL), ("yh", 13, np.nan), ("yh", 47, 0.5),
            ("out", 49, 0.0))
    for bad in bads:
        gy = np.full((rows, 64), G.SENTINEL, np.float32)
        go = np.full(rows, G.SENTINEL, np.float32)
        gy[:live], go[:live] = yh[:live], out[:live]
        if bad is None:
            G.compare(gy, go, yh, out, live, G.YH_TOL, G.OUT_TOL)
            continue
        arr, row, d = bad
        if arr == "yh":
            gy[row, 63] = gy[row, 63] + d if row < live else d
        else:
            go[row] = go[row] + d if row < live else d
        with pytest.raises(AssertionError):
            G.compare(gy, go, yh, out, live, G.YH_TOL, G.OUT_TOL)
