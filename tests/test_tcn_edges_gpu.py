"""Edges of the temporal-convolution kernels (csrc/kernels/conv1d.hip): a row's result against its
placement (bucket, position, time tile, staging mode, input source), the event-ring input, the live
row count, NaN / inf containment, the read-out kernel. Helpers: tests/test_tcn_gpu.py; cases and
reference: tests/tcn_cases.py."""
import numpy as np
import pytest

from tests import tcn_cases as C
from tests.test_tcn_gpu import CANARY, _ring_store, make_step, ref_layer, run_conv, seq_buf

pytestmark = pytest.mark.gpu


def _real_layer(rows, T, ci, co, k, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, T, ci)).astype(np.float32)
    w = (rng.standard_normal((co, ci, k)) / np.sqrt(ci * k)).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32)
    return x, w, b


# ------------------------------------------------------------------------------ placement
def test_a_rows_result_does_not_depend_on_its_placement():
    """Real-valued data, so the summation order shows: the same history gives bit-equal output in a
    launch of 1, 63 and 65 rows, at the first and the last position, with 32- and 64-step time tiles,
    staged once or per tap, and read as an activation buffer or as the dense model input."""
    T, ci, co, k, d = 100, 24, 40, 3, 4
    x, w, b = _real_layer(65, T, ci, co, k)
    s = make_step(w, b, d, 8, T, act="tanh")
    base = run_conv(s, x)[:65, :, :co]
    err = np.abs(base.astype(np.float64) - ref_layer(x, w, b, d, 8, "tanh")).max()
    assert 0 < err < 1e-5, err    # real data: not exact, and right
    for rows in (1, 63):
        assert np.array_equal(run_conv(s, x[:rows])[:rows, :, :co], base[:rows]), rows
    moved = np.ascontiguousarray(x[::-1])
    assert np.array_equal(run_conv(s, moved)[:65, :, :co], base[::-1])
    for kw in (dict(tt=32), dict(tt=64), dict(per_tap=True), dict(tt=32, per_tap=True), dict(dense=True)):
        assert np.array_equal(run_conv(s, x, **kw)[:65, :, :co], base), kw


def test_wide_layers_with_long_dilations_stage_per_tap():
    """C_in = 200 with dil (k - 1) = 128 does not fit tile + halo into the LDS: the per-tap staging runs
    by itself, bit-equal to float64 on integers, as do the limits C = 256, k = 8 on a short sequence."""
    rng = np.random.default_rng(3)
    for rows, T, ci, co, k, d in ((3, 40, 200, 20, 3, 64), (2, 9, 256, 256, 8, 1), (2, 70, 130, 17, 2, 128)):
        x, w, b = C.int_conv_case(rng, rows, T, ci, co, k, d)
        pl = d * (k - 1)
        Y = run_conv(make_step(w, b, d, pl, T), x)
        assert np.array_equal(Y[:rows, :, :co].astype(np.float64), ref_layer(x, w, b, d, pl)), (ci, co, k, d)


# ------------------------------------------------------------------------------ event rings
@pytest.mark.parametrize("T", [7, 100])
def test_event_ring_input(T):
    """The ring case of the GRU edge suite (ev_count 0, 1, T - 1, T, T + 1 and the ring, heads 0, 1 and
    ring - 1 - wrapped windows - and slot -1) at T = 7 below the 100-entry ring and at T = ring: a first
    layer reading the rings is bit-equal to the same layer fed the gathered histories as dense input,
    and to float64 on them within the real-data error."""
    import torch
    from igaming_platform_amd.ops import kernels as K
    store, X, slots = _ring_store(T)        # X [T, rows, 16]
    rows = len(slots)
    assert (slots == -1).any()
    _, w, b = _real_layer(1, T, 16, 33, 3, seed=T)
    s = make_step(w, b, 2, 4, T, act="relu")
    Y = torch.full((rows + 2, T, 40), CANARY, dtype=torch.float32).cuda()
    K.conv1d(s, rows, T, Y, store=store, slots=torch.from_numpy(slots).cuda())
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    xr = np.ascontiguousarray(X.transpose(1, 0, 2))
    dense = run_conv(s, xr, dense=True)
    assert np.array_equal(got[:rows, :, :33], dense[:rows, :, :33])
    assert (got[rows:] == CANARY).all()
    ref = ref_layer(xr, w, b, 2, 4, "relu")
    assert np.abs(got[:rows, :, :33] - ref).max() < 1e-5
    empty = np.nonzero(slots == -1)[0]
    assert np.array_equal(got[empty, :, :33], np.broadcast_to(np.maximum(b, 0), (len(empty), T, 33)))


# ------------------------------------------------------------------------------ live rows, NaN and inf
def test_rows_past_the_live_count_are_left_untouched():
    import torch
    rng = np.random.default_rng(1)
    x, w, b = C.int_conv_case(rng, 65, 17, 6, 9, 2, 1)
    s = make_step(w, b, 1, 1, 17)
    ref = ref_layer(x, w, b, 1, 1)
    for live in (0, 1, 64, 65, 200):
        Y = run_conv(s, x, m_ptr=torch.tensor([live], dtype=torch.int32).cuda())
        n = min(live, 65)
        assert np.array_equal(Y[:n, :, :9].astype(np.float64), ref[:n]), live
        assert (Y[n:] == CANARY).all(), live


def test_nan_and_inf_stay_in_their_own_row():
    rng = np.random.default_rng(4)
    x, w, b = C.int_conv_case(rng, 5, 40, 6, 20, 3, 2)
    clean = run_conv(make_step(w, b, 2, 4, 40), x)
    x2 = x.copy()
    x2[1, 20, 3], x2[3, 0, 0] = np.nan, np.inf
    Y = run_conv(make_step(w, b, 2, 4, 40), x2)
    for r in (0, 2, 4):
        assert np.array_equal(Y[r], clean[r]), r
    assert np.isnan(Y[1, :, :20]).any() and not np.isfinite(Y[3, :, :20]).all()
    assert (Y[:5, :, 20:32] == 0).all()     # the padding channels of the last block stay zero


# ------------------------------------------------------------------------------ the read-out
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 100])
def test_seq_pool(T):
    """last / mean / max / sum at the T edges, float32 and bfloat16 out: integers are exact (the mean is
    the correctly rounded quotient); a NaN in a column makes max NaN wherever it stands; rows past the
    live count and columns past C are left alone."""
    import torch
    from igaming_platform_amd.ops import kernels as K
    rng = np.random.default_rng(T)
    rows, Cn = 67, 19
    x = rng.integers(-8, 9, (rows, T, Cn)).astype(np.float32)
    x[2, 0, 1] = x[3, T - 1, 2] = x[4, T // 2, 3] = np.nan
    X = seq_buf(x)
    m_ptr = torch.tensor([rows - 1], dtype=torch.int32).cuda()
    xt = x.transpose(0, 2, 1)
    with np.errstate(invalid="ignore"):
        want = {"last": C.ref_pool(xt, "last"), "max": C.ref_pool(xt, "max"), "sum": C.ref_pool(xt, "sum"),
                "mean": (C.ref_pool(xt, "sum").astype(np.float32) / np.float32(T)).astype(np.float64)}
    assert np.isnan(want["max"][2, 1]) and np.isnan(want["max"][3, 2]) and np.isnan(want["max"][4, 3])
    for op, ref in want.items():
        for dt in (torch.float32, torch.bfloat16):
            Y = torch.full((rows + 1, Cn + 2), CANARY, dtype=dt).cuda()
            K.seq_pool(op, X, Y, rows, T, Cn, m_ptr=m_ptr)
            torch.cuda.synchronize()
            got = Y.float().cpu().numpy()
            assert (got[rows - 1:] == CANARY).all() and (got[:, Cn:] == CANARY).all(), (op, dt)
            exp = ref[:rows - 1]
            if dt == torch.bfloat16:
                exp = torch.from_numpy(exp.astype(np.float32)).to(torch.bfloat16).float().numpy()
            np.testing.assert_array_equal(got[:rows - 1, :Cn], exp.astype(np.float32), err_msg=f"{op} {dt}")
