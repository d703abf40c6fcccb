"""K4 LSTM (lstm.hip: all 24 instances of lstm_kernel<RT, KSX, KSH, NW, SPLIT>) on every dispatch path
against the float64 reference of tests/lstm_cases.py, at the tolerances that file measures on the
reference alone.

Every launch writes Y_h and the head's score together into buffers pre-filled with -7, three rows
longer than the launch; X is 50 rows wide and its rows at and past the live count are NaN. The bf16
kernels are held to the bf16-rounding reference (YH_TOL / OUT_TOL), the f32-faithful ones to the
unrounded reference at 1e-4; a 32-row launch must equal the 16-row launch bit for bit. Which instances
the tables reach is asserted in tests/test_lstm_edges.py.

Measured gaps to the reference on an MI355X (max over the cases of a family):

| family                                        | yh      | out     | bound (yh / out)    |
|-----------------------------------------------|---------|---------|---------------------|
| lstm_kernel<.., 0>, dense                     | 6.36e-5 | 7.50e-4 | 1.87e-4 / 3.01e-3   |
| lstm_kernel<.., 0>, dense, head without sigmoid | 1.09e-7 | 4.75e-6 | 1.87e-4 / 1.02e-5 |
| lstm_kernel<.., 1>, dense                     | 2.80e-6 | 2.10e-5 | 1e-4 / 1e-4         |
| lstm_kernel<.., 1>, dense, head without sigmoid | 1.13e-6 | 4.96e-5 | 1e-4 / 1e-4       |
| event rings, bf16 kernels                     | 2.14e-5 | 1.86e-4 | 1.87e-4 / 3.01e-3   |
| event rings, f32-faithful kernels             | 2.77e-7 | 2.15e-6 | 1e-4 / 1e-4         |
| bidirectional layer, fp32 plan                | 2.84e-6 | 1.35e-5 | 1e-4 / 1e-4         |

All 158 pairs of a 32-row and a 16-row launch (150 dense, 8 over the rings) were equal bit for bit in
Y_h and the score.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import lstm_cases as L

pytestmark = pytest.mark.gpu

PAD = 3  # output rows past the launch
GAPS = {}


def _t():
    import torch
    return torch


def _K():
    from igaming_platform_amd.ops import kernels as K
    return K


def _note(family, g):
    cur = GAPS.setdefault(family, [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], g[0]), max(cur[1], g[1])
    print(f"gap {family}: yh {cur[0]:.2e} out {cur[1]:.2e}")


@lru_cache(maxsize=None)
def _pack(name, split, reverse):
    ls, head = L.plan_steps(name)
    return _K().LstmPack(ls, head, "cuda", split=split, reverse=reverse)


@lru_cache(maxsize=None)
def _x(name, live):
    return _t().from_numpy(L.nan_past(L.dense_x(name), live)).cuda()


def _ref(name, reverse, bf16):
    return L.reference(f"{name}-dense" + ("-reverse" if reverse else ""), bf16)


def _buffers(n_rows, H):
    torch = _t()
    return (torch.full((n_rows + PAD, H), L.SENTINEL, dtype=torch.float32, device="cuda"),
            torch.full((n_rows + PAD,), L.SENTINEL, dtype=torch.float32, device="cuda"))


def _launch(lp, T, n_rows, live, **kw):
    """One K.lstm launch into sentinel buffers -> (yh [n_rows + PAD, H], out [n_rows + PAD]) numpy."""
    torch = _t()
    yh, out = _buffers(n_rows, lp.H)
    m_ptr = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    _K().lstm(lp, n_rows, T, out=out, yh=yh, m_ptr=m_ptr, **kw)
    torch.cuda.synchronize()
    return yh.cpu().numpy(), out.cpu().numpy()


def _ids(names, reverse_too):
    return [(n, False) for n in names] + [(n, True) for n in reverse_too]


def _dense_paths(name, reverse, split, family):
    """Every row pair x tile size of one model: against the reference, and 32-row == 16-row."""
    m = L.MODELS[name]
    lp = _pack(name, split, reverse)
    ryh, rout = _ref(name, reverse, not split)
    tol = (L.SPLIT_TOL, L.SPLIT_TOL) if split else L.tol(name)
    if m.act == "none":
        family += ", no sigmoid"
    paths = L.paths(name, split)
    assert [inst[0] for _, inst in paths] == [1, 2]
    for n_rows, live in L.BP_LIVE:
        lv = n_rows if live is None else live
        Xd = _x(name, lv)
        assert Xd.shape[1] == L.BP_XROWS > n_rows
        got = []
        for opts, inst in paths:
            what = f"{name} reverse={reverse} lstm_kernel{inst} rows {n_rows} live {live}"
            yh, out = _launch(lp, m.T, n_rows, live, X=Xd, **opts)
            _note(family, L.compare(yh, out, ryh, rout, lv, *tol, what))
            got.append((yh, out))
        assert np.array_equal(got[0][0], got[1][0]), f"{name} rows {n_rows} live {live}: yh of the 32-row tiles differs"
        assert np.array_equal(got[0][1], got[1][1]), f"{name} rows {n_rows} live {live}: out of the 32-row tiles differs"


# ------------------------------------------------------------------------------ dense input
@pytest.mark.parametrize("name,reverse", _ids(list(L.MODELS), L.REVERSE_MODELS))
def test_bf16_paths_match_the_reference(name, reverse):
    """lstm_kernel<1 | 2, KSX, KSH, NW, 0> against the bf16 reference, at 47 of 50 rows with live
    counts of 47, 33, 16 and 0 and at one row; the 32-row launch equals the 16-row one bit for bit."""
    _dense_paths(name, reverse, False, "bf16 dense")


@pytest.mark.parametrize("name,reverse", _ids(list(L.MODELS), L.REVERSE_MODELS))
def test_split_paths_match_float64(name, reverse):
    """lstm_kernel<1 | 2, KSX, KSH, NW, 1> against the unrounded float64 reference at 1e-4, the same
    rows; the 32-row launch equals the 16-row one bit for bit."""
    _dense_paths(name, reverse, True, "split dense")


def test_tile_rows_binding_matches_the_mirror():
    """lstm_tile_rows (what LstmPack's callers size their launches by) against the mirror's LDS check,
    for every (H, input padding, split) at a request of 32 - the 24 instances - and of 16 and 0."""
    from igaming_platform_amd.native import hipk
    seen = set()
    for m in L.MODELS.values():
        for split in (0, 1):
            kx = 32 if m.I <= 32 else 64
            for req in (32, 16, 0):
                inst = L.dispatch(m, req, bool(split))
                assert hipk().lstm_tile_rows(m.H, kx, split, req) == 16 * inst[0], (m.name, split, req)
                seen.add(inst)
            assert hipk().lstm_tile_rows(m.H, kx, split, 32) == 32 and hipk().lstm_tile_rows(m.H, kx, split, 16) == 16
    assert len(seen) == 24


# ------------------------------------------------------------------------------ event rings
@lru_cache(maxsize=None)
def _store(T):
    torch = _t()
    from igaming_platform_amd.config import FeatureConfig
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.layouts import ACCTRT
    fc = FeatureConfig()
    fc.event_ring = L.RING
    ev, head, count, slots = L.ring_case(T, fc.event_dim)
    C = ev.shape[0]
    store = DeviceFeatureStore(C, fc, "cuda", events=True, max_events=64)
    assert tuple(store.ev.shape) == ev.shape
    store.ev.copy_(torch.from_numpy(ev).to(torch.bfloat16).view(torch.int16).cuda())
    rt = np.zeros(C, ACCTRT)
    rt["ev_head"], rt["ev_count"] = head, count
    store.rt.copy_(torch.from_numpy(rt.view(np.int32).reshape(C, -1).copy()).cuda())
    return store, torch.from_numpy(slots).cuda()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", L.RING_T)
def test_event_rings(T, reverse, split):
    """Model E from the HBM event rings at T = 7 on the 12-entry ring and at T = ring: ev_count 0, 3,
    T and ring, heads that wrap, empty and repeated slots, 48 rows, at both tile sizes. The ring holds
    bf16 values, so x is exact and the tolerances are those of dense input. A row with an empty
    history equals the all-zero sequence bit for bit."""
    torch = _t()
    store, slots = _store(T)
    label = f"E-ring-{T}" + ("-reverse" if reverse else "")
    rows = L.RING_ROWS
    lp = _pack("E", split, reverse)
    ryh, rout = L.reference(label, not split)
    tol = (L.SPLIT_TOL, L.SPLIT_TOL) if split else L.tol("E")
    zeros = torch.zeros((T, 1, lp.I), dtype=torch.float32, device="cuda")
    empty = L.ring_empty_rows(T)
    got = []
    for opts, inst in L.paths("E", split):
        what = f"{label} lstm_kernel{inst}"
        yh, out = _launch(lp, T, rows, None, store=store, slots=slots, **opts)
        _note("ring split" if split else "ring bf16", L.compare(yh, out, ryh, rout, rows, *tol, what))
        zyh, zout = _launch(lp, T, 1, None, X=zeros, **opts)
        for b in empty:
            assert np.array_equal(yh[b], zyh[0]) and out[b] == zout[0], f"{what}: empty row {b} is not the zero sequence"
        got.append((yh, out))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), f"{label}: tiles differ"


# ------------------------------------------------------------------------------ bidirectional
@pytest.mark.parametrize("head", [True, False])
@pytest.mark.parametrize("name", list(L.BI_MODELS))
def test_bidirectional_model(name, head):
    """One bidirectional layer through LstmModel on the fp32 plan (a forward and a reverse split launch,
    the head as a dense launch over [rows, 2H]) at T = 3, rows 1 and 47 of 50: Y_h in [N, 2, H] order
    and the score against float64 at 1e-4; nothing past the launch is written. No m_ptr: with one, the
    headless path copies whole rows through torch.cat, which is outside this suite."""
    torch = _t()
    from igaming_platform_amd.engine.runner import LstmModel
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import native
    m = L.BI_MODELS[name]
    plan = to_device(compile_onnx(native().OnnxModel.from_bytes(L.onnx_bilstm(name, head))), "cuda", "fp32")
    lm = LstmModel(plan.steps, "cuda", True, L.BP_XROWS)
    assert lm.bidirectional and lm.split and lm.has_head == head
    X = L.dense_x(name)
    ryh, rout = L.bi_ref(name, X, head)
    ref = rout[:, None] if head else ryh
    sent = np.float32(L.SENTINEL).view(np.int32)
    for rows in L.BI_ROWS:
        Xd = torch.from_numpy(L.nan_past(X, rows)).cuda()
        out = torch.full((rows + PAD, 1 if head else 2 * m.H), L.SENTINEL, dtype=torch.float32, device="cuda")
        lm.run(rows, m.T, out, X=Xd)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[rows:].view(np.int32) == sent), f"{name} rows {rows}: written past the launch"
        assert not np.isnan(got[:rows]).any()
        g = float(np.abs(got[:rows] - ref[:rows]).max())
        _note("bidirectional", (0.0, g) if head else (g, 0.0))
        assert g <= L.SPLIT_TOL, f"{name} head={head} rows {rows}: off by {g:.3e}"
        if head:  # the head reads the [N, 2, H] order: both halves of the buffer it ran over
            cat = lm.cat[:rows].cpu().numpy()
            gc = float(np.abs(cat - ryh[:rows]).max())
            _note("bidirectional", (gc, 0.0))
            assert gc <= L.SPLIT_TOL, f"{name} rows {rows}: Y_h off by {gc:.3e}"


# ------------------------------------------------------------------------------ operand checks
def test_lstm_validates_operands():
    """What K.lstm refuses before any launch (the buffers keep their fill)."""
    torch = _t()
    K = _K()
    lp = _pack("E", False, False)
    ls, _ = L.plan_steps("E")
    headless = K.LstmPack(ls, None, "cuda")
    T, rows = L.MODELS["E"].T, 20
    X = _x("E", L.BP_XROWS)
    yh, out = _buffers(rows, lp.H)
    store, slots = _store(7)
    bad = [
        dict(lp=lp, T=T, X=X, out=out, yh=yh, tile_rows=8),
        dict(lp=lp, T=0, X=X, out=out, yh=yh),
        dict(lp=lp, T=T, X=X[:, :, :8].contiguous(), out=out, yh=yh),      # wrong width
        dict(lp=lp, T=T, X=X[:, :rows - 1].contiguous(), out=out, yh=yh),  # fewer rows than the launch
        dict(lp=lp, T=T, X=X[:T - 1], out=out, yh=yh),                     # fewer steps than T
        dict(lp=lp, T=L.RING + 1, store=store, slots=slots, out=out, yh=yh),  # a ring shorter than T
        dict(lp=lp, T=T, X=X, yh=yh),                                      # a head without out
        dict(lp=headless, T=T, X=X, out=out),                              # neither head nor yh
        dict(lp=lp, T=T, out=out, yh=yh),                                  # no input at all
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises((ValueError, RuntimeError), match="lstm"):
            K.lstm(kw.pop("lp"), rows, kw.pop("T"), **kw)
    torch.cuda.synchronize()
    assert bool(torch.all(yh == L.SENTINEL)) and bool(torch.all(out == L.SENTINEL))
    K.lstm(lp, rows, T, X=X, out=out, yh=yh)  # and the same operands, valid, launch
    torch.cuda.synchronize()
    assert bool(torch.all(out[:rows] != L.SENTINEL)) and bool(torch.all(out[rows:] == L.SENTINEL))
