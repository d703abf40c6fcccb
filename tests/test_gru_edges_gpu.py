"""K4 (gru.hip: gru_kernel, gru2_pipe_kernel, gru_x3_kernel; gru_ws.hip: gru_ws_kernel<false / true>,
gru_ws2_kernel; gru_wsx.hip) on every dispatch path against the float64 reference of
tests/gru_cases.py, at the tolerances that file measures on the reference alone.

Every launch writes Y_h and the head's score into buffers pre-filled with -7, three rows longer than
the launch; X rows at and past the live count are NaN. The bf16 kernels are held to the bf16-rounding
reference (YH_TOL / OUT_TOL), the f32-faithful ones to the unrounded reference at 1e-4. The other
bf16 batch-parallel instances of a model must also equal its default path: Y_h bit for bit, the score
to 1e-6 (the head's cross-wave sum order). Which instances the tables reach is asserted in
tests/test_gru_edges.py.

Measured gaps to the reference on an MI355X (max over the cases of a family):

| family                                   | yh      | out     | bound (yh / out)  |
|------------------------------------------|---------|---------|-------------------|
| gru_kernel / gru2_pipe_kernel, dense     | 1.54e-4 | 8.42e-4 | 4.6e-4 / 1.9e-3   |
| gru_x3_kernel, dense                     | 5.52e-6 | 1.60e-5 | 1e-4 / 1e-4       |
| gru_ws_kernel<false / true>, gru_ws2     | 8.04e-5 | 3.28e-4 | 4.6e-4 / 1.9e-3   |
| gru_wsx_kernel                           | 1.19e-6 | 7.29e-6 | 1e-4 / 1e-4       |
| event rings, bf16 kernels                | 9.34e-5 | 4.35e-4 | 4.6e-4 / 1.9e-3   |
| event rings, f32-faithful kernels        | 8.08e-7 | 3.87e-6 | 1e-4 / 1e-4       |

All 368 (instance, row count) pairs of a bf16 path and its model's default path had bit-equal Y_h; their
scores differed by at most 4.17e-7.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import gru_cases as G

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
    gs, head = G.plan_steps(name)
    return _K().GruPack(gs, head, "cuda", split=split, reverse=reverse)


@lru_cache(maxsize=None)
def _x(name, live, x_rows):
    return _t().from_numpy(G.nan_past(G.dense_x(name), live, x_rows)).cuda()


def _ref(name, reverse, bf16):
    return G.reference(f"{name}-dense" + ("-reverse" if reverse else ""), bf16)


def _launch(gp, T, n_rows, live, **kw):
    """One K.gru launch into sentinel buffers -> (yh [n_rows + PAD, H], out [n_rows + PAD]) numpy."""
    torch = _t()
    yh = torch.full((n_rows + PAD, gp.H), G.SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((n_rows + PAD,), G.SENTINEL, dtype=torch.float32, device="cuda")
    m_ptr = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    _K().gru(gp, n_rows, T, out=out, yh=yh, m_ptr=m_ptr, **kw)
    torch.cuda.synchronize()
    return yh.cpu().numpy(), out.cpu().numpy()


def _ids(names, reverse_too):
    return [(n, False) for n in names] + [(n, True) for n in reverse_too]


# ------------------------------------------------------------------------------ batch-parallel, bf16
@pytest.mark.parametrize("name,reverse", _ids(list(G.MODELS), G.REVERSE_MODELS))
def test_bf16_paths_match_the_reference_and_the_default_path(name, reverse):
    """The model's default path (tile 16, layer-pipelined when two layers, default waves) against the
    bf16 reference; every other instance (32-row tiles, pipeline = 0, waves = 4, their combinations)
    against the reference and the default path, at 47 of 50 rows with live counts of 47, 33, 16 and at
    one row."""
    m = G.MODELS[name]
    gp = _pack(name, False, reverse)
    ryh, rout = _ref(name, reverse, True)
    for n_rows, live in G.BP_LIVE:
        lv = n_rows if live is None else live
        Xd = _x(name, lv, G.BP_XROWS)
        anchor = None
        for opts, inst in G.bf16_paths(name):
            what = f"{name} reverse={reverse} {inst} rows {n_rows} live {live}"
            yh, out = _launch(gp, m.T, n_rows, live, X=Xd, ws=0, **opts)
            _note("bf16 dense", G.compare(yh, out, ryh, rout, lv, G.YH_TOL, G.OUT_TOL, what))
            if anchor is None:
                anchor = (yh, out)
            elif (name, inst) not in G.NOT_BIT_EQUAL:
                d = float(np.abs(out[:lv] - anchor[1][:lv]).max())
                print(f"{what}: yh equal {np.array_equal(yh, anchor[0])}, out gap {d:.2e}")
                assert np.array_equal(yh, anchor[0]), f"{what}: yh differs from the default path"
                assert d <= G.HEAD_ORDER_TOL, f"{what}: out {d:.3e} from the default path"


# ------------------------------------------------------------------------------ batch-parallel, split
@pytest.mark.parametrize("name,reverse", _ids(list(G.MODELS), G.REVERSE_MODELS))
def test_split_paths_match_float64(name, reverse):
    """gru_x3_kernel at 16- and (lbr = 1) 32-row tiles, 8 and 16 waves at H = 256, against the
    unrounded float64 reference at 1e-4; a 32-row instance equals its 16-row twin bit for bit."""
    m = G.MODELS[name]
    gp = _pack(name, True, reverse)
    ryh, rout = _ref(name, reverse, False)
    for n_rows, live in G.BP_LIVE:
        lv = n_rows if live is None else live
        Xd = _x(name, lv, G.BP_XROWS)
        got = {}
        for opts, inst in G.split_paths(name):
            what = f"{name} reverse={reverse} {inst} rows {n_rows} live {live}"
            yh, out = _launch(gp, m.T, n_rows, live, X=Xd, ws=0, **opts)
            _note("split dense", G.compare(yh, out, ryh, rout, lv, G.SPLIT_TOL, G.SPLIT_TOL, what))
            got[inst] = (yh, out)
        for inst, (yh, out) in got.items():
            twin = (inst[0], 1) + inst[2:]
            if inst[1] == 2 and twin in got:
                assert np.array_equal(yh, got[twin][0]) and np.array_equal(out, got[twin][1]), f"{inst} != {twin}"


# ------------------------------------------------------------------------------ cluster kernels
@pytest.mark.parametrize("ws", list(G.CLUSTER_ROWS))
@pytest.mark.parametrize("name,reverse", _ids(G.CLUSTER_MODELS, ["E"]))
def test_cluster_kernels_match_the_reference(name, reverse, ws):
    """gru_ws_kernel<false / true> (ws 1 / 2), gru_ws2_kernel (ws 3) against the bf16 reference and
    gru_wsx_kernel against float64 at 1e-4: one row, one row short of a cluster, one past it, a live
    count that ends inside a cluster; T = 1, 2, 3 (E_T*) and 1, 2, 4 input chunks (E8, E, E32). Each
    launch runs twice (the counters return to 0), writes the head partials of its workspace (only a
    cluster kernel does) and reports no timeout."""
    torch = _t()
    m = G.MODELS[name]
    split = ws == "wsx"
    gp = _pack(name, split, reverse)
    assert gp.wsx_ok if split else gp.ws_ok
    ryh, rout = _ref(name, reverse, not split)
    tol = (G.SPLIT_TOL, G.SPLIT_TOL) if split else (G.YH_TOL, G.OUT_TOL)
    for n_rows, live in G.CLUSTER_ROWS[ws]:
        lv = n_rows if live is None else live
        Xd = _x(name, lv, n_rows + PAD)
        wsp = gp.workspace(n_rows)
        wsp["part"].zero_()
        first = None
        for _ in range(2):
            what = f"{name} reverse={reverse} {G.CLUSTER_KERNEL[ws]} rows {n_rows} live {live}"
            yh, out = _launch(gp, m.T, n_rows, live, X=Xd, ws=3 if split else ws)
            assert not gp.ws_failed(), what
            _note("wsx" if split else "ws", G.compare(yh, out, ryh, rout, lv, *tol, what))
            assert int(wsp["sync"].abs().sum()) == 0, f"{what}: counters not back at 0"
            if first is None:
                first = (yh, out)
            else:
                assert np.array_equal(yh, first[0]) and np.array_equal(out, first[1]), f"{what}: second launch differs"
        assert bool(torch.any(wsp["part"] != 0)), f"{what}: the cluster kernel did not run"


# ------------------------------------------------------------------------------ event rings
@lru_cache(maxsize=None)
def _store(T):
    torch = _t()
    from igaming_platform_amd.config import FeatureConfig
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.layouts import ACCTRT
    fc = FeatureConfig()
    ev, head, count, slots = G.ring_case(fc.event_ring, fc.event_dim, T)
    C = ev.shape[0]
    store = DeviceFeatureStore(C, fc, "cuda", events=True, max_events=64)
    store.ev.copy_(torch.from_numpy(ev).to(torch.bfloat16).view(torch.int16).cuda())
    rt = np.zeros(C, ACCTRT)
    rt["ev_head"], rt["ev_count"] = head, count
    store.rt.copy_(torch.from_numpy(rt.view(np.int32).reshape(C, -1).copy()).cuda())
    return store, torch.from_numpy(slots).cuda()


RING_PATHS = [
    ("default", False, dict(ws=0, tile_rows=16)),
    ("32-row", False, dict(ws=0, tile_rows=32)),
    ("unpipelined", False, dict(ws=0, tile_rows=32, pipeline=0)),
    ("ws1", False, dict(ws=1)),
    ("ws2", False, dict(ws=2)),
    ("ws3", False, dict(ws=3)),
    ("split", True, dict(ws=0, tile_rows=16)),
    ("split 32-row", True, dict(ws=0, tile_rows=32)),
    ("wsx", True, dict(ws=3)),
]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", G.RING_T)
def test_event_rings(T, reverse):
    """Model E from the HBM event rings at T = 7 on the 100-entry ring and at T = ring: ev_count 0, 1,
    T - 1, T, T + 1 and ring, ev_head 0, 1 and ring - 1, empty slots; on the default path, a 32-row
    path, the un-pipelined kernel, every cluster kernel and the f32-faithful kernels, forward and
    reverse. The ring holds bf16 values, so x is exact and the tolerances are those of dense input."""
    Tn, _ = G.ring_x(T)
    store, slots = _store(Tn)
    label = f"E-ring-{T}" + ("-reverse" if reverse else "")
    rows = G.RING_ROWS
    for path, split, opts in RING_PATHS:
        gp = _pack("E", split, reverse)
        ryh, rout = G.reference(label, not split)
        tol = (G.SPLIT_TOL, G.SPLIT_TOL) if split else (G.YH_TOL, G.OUT_TOL)
        what = f"{label} {path}"
        wsp = gp.workspace(rows) if opts["ws"] else None
        if wsp is not None:
            wsp["part"].zero_()
        yh, out = _launch(gp, Tn, rows, None, store=store, slots=slots, **opts)
        assert not gp.ws_failed(), what
        _note("ring split" if split else "ring bf16", G.compare(yh, out, ryh, rout, rows, *tol, what))
        if wsp is not None:
            assert bool(_t().any(wsp["part"] != 0)), f"{what}: the cluster kernel did not run"
