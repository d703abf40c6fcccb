"""Per-sequence lengths (ONNX sequence_lens) in the K4 kernels on the device: the masked instances of
gru_kernel, gru2_pipe_kernel, gru_x3_kernel and lstm_kernel against the per-row float64 reference of
tests/seqlen_cases.py, at the bounds of the edge suites (conditions: tests/test_seqlen.py).

Every launch writes Y_h and the head's score into buffers pre-filled with -7, three rows longer than
the launch; X rows at and past the live count are NaN. Besides the comparisons with the reference the
file holds exact checks: a masked launch with every length T equals the unmasked launch of the same
instance bit for bit, one with every length L equals the unmasked launch at T = L, a 32-row tile
equals the 16-row one in Y_h, and a launch from the event rings equals the dense launch fed the
left-aligned gather. (Comparisons go through lstm_cases.compare for both cells: it is
gru_cases.compare with a live count of 0 allowed.)

Measured gaps to the reference on an MI355X (max over the cases of a family; bounds as in the edge suites):

| family                                  | yh      | out     | bound (yh / out)   |
|-----------------------------------------|---------|---------|--------------------|
| gru_kernel / gru2_pipe_kernel, dense    | 7.70e-5 | 2.82e-4 | 4.6e-4 / 1.9e-3    |
| gru_x3_kernel, dense                    | 4.49e-6 | 2.57e-5 | 1e-4 / 1e-4        |
| lstm_kernel SPLIT = 0, dense            | 2.33e-5 | 1.38e-4 | 1.87e-4 / 3.01e-3  |
| lstm_kernel SPLIT = 1, dense            | 1.06e-6 | 6.87e-6 | 1e-4 / 1e-4        |
| event rings, bf16 GRU / LSTM            | 9.11e-5 | 1.86e-4 | as dense           |
| event rings, f32-faithful GRU / LSTM    | 7.30e-7 | 2.35e-6 | 1e-4 / 1e-4        |

AbuseGpu on the masked cfg5-shaped model: 2.98e-8 from the CPU engine's scores.

What notices a missing select: with `if constexpr (MASKED != 0) h = live(rt, r) ? h : hs...` taken out of
layer_step's linear_before_reset = 1 branch (a scratch build), 21 tests of this file fail - the dense
comparisons of gru-A, gru-A-32, gru-E-unpiped-32, pipe-E, pipe-E-32, pipe-E-T1 / T2 / T3, the uniform-length
checks of the five T = 7 cases among them, both GRU event-ring tests and the bf16 bidirectional GRU.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import gru_cases as G
from tests import lstm_cases as L
from tests import seqlen_cases as Q

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
def _pack(kind, name, split, reverse, masked):
    K = _K()
    c = next(c for c in Q.CASES if c.kind == kind and c.model == name)
    steps, head = Q.steps(c) if masked else Q.table(kind).plan_steps(name)
    gp = (K.GruPack if kind == "gru" else K.LstmPack)(steps, head, "cuda", split=split, reverse=reverse)
    assert gp.masked == masked
    return gp


def _case_pack(c, masked=True):
    return _pack(c.kind, c.model, c.split, c.reverse, masked)


def _dev(a):
    return _t().from_numpy(np.array(a)).cuda()   # a copy: the cached case arrays are read-only


def _launch(kind, gp, T, n_rows, live, **kw):
    """One K.gru / K.lstm launch into sentinel buffers -> (yh [n_rows + PAD, H], out [n_rows + PAD]) numpy."""
    torch = _t()
    yh = torch.full((n_rows + PAD, gp.H), G.SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.full((n_rows + PAD,), G.SENTINEL, dtype=torch.float32, device="cuda")
    m_ptr = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    if kind == "gru":
        kw.setdefault("ws", 0)
        _K().gru(gp, n_rows, T, out=out, yh=yh, m_ptr=m_ptr, **kw)
    else:
        _K().lstm(gp, n_rows, T, out=out, yh=yh, m_ptr=m_ptr, **kw)
    torch.cuda.synchronize()
    return yh.cpu().numpy(), out.cpu().numpy()


def _nan_past(X, live):
    X = np.array(X)
    X[:, live:] = np.nan
    return X


# ------------------------------------------------------------------------------ dense input
@pytest.mark.parametrize("cid", [c.id for c in Q.CASES])
def test_masked_launch_matches_the_per_row_reference(cid):
    """47 rows inside a 50-row X, live counts 47 / 33 / 0 through m_ptr, lengths that differ inside
    every accumulator group and MFMA tile; rows past the live count stay untouched."""
    c = Q.BY_ID[cid]
    gp = _case_pack(c)
    assert not gp.ws_ok and not gp.wsx_ok
    ryh, rout = Q.reference(cid)
    lens = _dev(Q.case_lens(c))
    for live in Q.LIVE:
        lv = Q.ROWS if live is None else live
        X = _dev(_nan_past(Q.case_x(cid), lv))
        what = f"{cid} {Q.instance(c)} live {live}"
        yh, out = _launch(c.kind, gp, c.T, Q.ROWS, live, X=X, lens=lens, **c.opts)
        fam = ("split " if c.split else "bf16 ") + c.kind
        _note(fam, L.compare(yh, out, ryh, rout, lv, *Q.tol(c), what))


@pytest.mark.parametrize("cid", [c.id for c in Q.CASES])
def test_full_length_is_bit_equal_to_the_unmasked_instance(cid):
    """Every length T (given, and lens = None): the masked instance computes what its unmasked twin does."""
    c = Q.BY_ID[cid]
    X = _dev(Q.case_x(cid))
    ref = _launch(c.kind, _case_pack(c, False), c.T, Q.ROWS, None, X=X, **c.opts)
    full = _dev(np.full(Q.XROWS, c.T, np.int32))
    for lens in (full, None):
        got = _launch(c.kind, _case_pack(c), c.T, Q.ROWS, None, X=X, lens=lens, **c.opts)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"{cid} lens {lens is not None}"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cid", [c.id for c in Q.CASES if c.T == Q.T])
def test_uniform_length_is_bit_equal_to_the_unmasked_launch_at_that_length(cid, n):
    """Every row of length L: the T - L held steps change nothing, forward and reverse."""
    c = Q.BY_ID[cid]
    Xn = np.array(Q.case_x(cid))
    Xn[n:] = np.nan     # a held step may read these, and must not let them through
    ref = _launch(c.kind, _case_pack(c, False), n, Q.ROWS, None, X=_dev(Q.case_x(cid)[:n]), **c.opts)
    got = _launch(c.kind, _case_pack(c), c.T, Q.ROWS, None, X=_dev(Xn), lens=_dev(np.full(Q.XROWS, n, np.int32)),
                  **c.opts)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"{cid} L = {n}"


@pytest.mark.parametrize("cid", [c.id for c in Q.CASES if c.id + "-32" in Q.BY_ID])
def test_32_row_tiles_equal_16_row_tiles_in_yh(cid):
    a, b = Q.BY_ID[cid], Q.BY_ID[cid + "-32"]
    assert (a.kind, a.model, a.split, a.reverse, a.T) == (b.kind, b.model, b.split, b.reverse, b.T)
    X, lens = _dev(Q.case_x(cid)), _dev(Q.case_lens(a))
    y16, o16 = _launch(a.kind, _case_pack(a), a.T, Q.ROWS, None, X=X, lens=lens, **a.opts)
    y32, o32 = _launch(b.kind, _case_pack(b), b.T, Q.ROWS, None, X=X, lens=lens, **b.opts)
    assert np.array_equal(y16, y32), f"{cid}: the 32-row tile's yh differs"
    assert float(np.abs(o16[:Q.ROWS] - o32[:Q.ROWS]).max()) <= G.HEAD_ORDER_TOL


# ------------------------------------------------------------------------------ event rings
@lru_cache(maxsize=None)
def _store(kind):
    torch = _t()
    from igaming_platform_amd.config import FeatureConfig
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.layouts import ACCTRT
    fc = FeatureConfig()
    if kind == "gru":
        case = G.ring_case(fc.event_ring, fc.event_dim, Q.T)
    else:
        fc.event_ring = L.RING
        case = L.ring_case(Q.T, fc.event_dim)
    ev, head, count, slots = case
    C = ev.shape[0]
    store = DeviceFeatureStore(C, fc, "cuda", events=True, max_events=64)
    assert tuple(store.ev.shape) == ev.shape
    store.ev.copy_(torch.from_numpy(ev).to(torch.bfloat16).view(torch.int16).cuda())
    rt = np.zeros(C, ACCTRT)
    rt["ev_head"], rt["ev_count"] = head, count
    store.rt.copy_(torch.from_numpy(rt.view(np.int32).reshape(C, -1).copy()).cuda())
    lens = np.array([0 if s < 0 else min(int(count[s]), Q.T) for s in slots], np.int32)
    gather = (G if kind == "gru" else L).ring_gather(ev, head, count, slots, Q.T)
    return store, torch.from_numpy(slots).cuda(), lens, Q.left_align(gather, lens)


RING_PATHS = {
    "gru": [("default", False, dict(tile_rows=16)), ("32-row", False, dict(tile_rows=32)),
            ("unpipelined", False, dict(tile_rows=32, pipeline=0)), ("clusters asked for", False, dict(ws=3)),
            ("split", True, dict(tile_rows=16)), ("split 32-row", True, dict(tile_rows=32)),
            ("split, clusters asked for", True, dict(ws=3))],
    "lstm": [("default", False, dict(tile_rows=16)), ("32-row", False, dict(tile_rows=32)),
             ("split", True, dict(tile_rows=16)), ("split 32-row", True, dict(tile_rows=32))],
}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_event_rings(kind, reverse):
    """Model E at T = 7 from the ring fixtures of the edge suites (ev_count 0 .. ring, wrapped heads,
    slot -1): the window comes from ev_count. Against the reference on the gathered histories with
    lens = min(ev_count, T), and bit-equal to the dense launch fed the left-aligned gather. A GRU
    launch that asks for the cluster kernels (the cluster shape) still takes the batch-parallel ones."""
    store, slots, lens, Xl = _store(kind)
    layers, head = Q.table(kind).weights("E")
    rows = len(lens)
    assert {0, 1, Q.T - 1, Q.T} <= set(lens) if kind == "gru" else {0, 3, Q.T} <= set(lens)
    for path, split, opts in RING_PATHS[kind]:
        gp = _pack(kind, "E", split, reverse, True)
        assert not gp.ws_ok and not gp.wsx_ok and (kind == "lstm" or gp.workspace(rows) is None)
        ryh, rout = Q.masked_ref(kind, layers, head, Xl, lens, reverse, not split)
        t = (Q.table(kind).SPLIT_TOL,) * 2 if split else ((G.YH_TOL, G.OUT_TOL) if kind == "gru" else L.tol("E"))
        what = f"{kind} ring reverse={reverse} {path}"
        yh, out = _launch(kind, gp, Q.T, rows, None, store=store, slots=slots, **opts)
        _note(f"ring {'split' if split else 'bf16'} {kind}", L.compare(yh, out, ryh, rout, rows, *t, what))
        dy, do = _launch(kind, gp, Q.T, rows, None, X=_dev(Xl), lens=_dev(lens), **opts)
        assert np.array_equal(yh, dy) and np.array_equal(out, do), f"{what}: differs from the dense launch"


# ------------------------------------------------------------------------------ runners
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("kind", ["gru", "lstm"])
def test_bidirectional_model_through_the_runner(kind, split):
    """One bidirectional layer with sequence_lens through GruModel / LstmModel (a forward and a
    reverse masked launch); without lens every row is full length."""
    torch = _t()
    from igaming_platform_amd.engine.runner import sequence_model
    from igaming_platform_amd.models.plan import compile_onnx
    from igaming_platform_amd.native import native
    plan = compile_onnx(native().OnnxModel.from_bytes(Q.bi_onnx(kind)))
    assert plan.lens_input == "sequence_lens"
    mdl = sequence_model(plan.steps, torch.device("cuda", 0), split, Q.XROWS)
    assert mdl.masked and mdl.bidirectional
    H2 = 2 * Q.BI[kind][1]
    X = _dev(Q.bi_x(kind))
    tol = Q.table(kind).SPLIT_TOL if split else Q.table(kind).YH_TOL
    for lens in (Q.lens_for(Q.XROWS, Q.T, 2), None):
        out = torch.full((Q.XROWS, H2), G.SENTINEL, dtype=torch.float32, device="cuda")
        mdl.run(Q.ROWS, Q.T, out, X=X, lens=None if lens is None else _dev(lens))
        torch.cuda.synchronize()
        ref = Q.bi_ref(kind, np.full(Q.XROWS, Q.T) if lens is None else lens, bf16=not split)
        got = out.cpu().numpy()
        gap = float(np.abs(got[:Q.ROWS] - ref[:Q.ROWS]).max())
        print(f"bidirectional {kind} split={split} lens={lens is not None}: gap {gap:.2e}")
        assert gap <= tol
        assert np.all(got[Q.ROWS:] == np.float32(G.SENTINEL))


# ------------------------------------------------------------------------------ services
def test_abuse_gpu_with_a_masked_model_matches_the_cpu_engine():
    """CheckBonusAbuse on backend="gpu" with the masked cfg5-shaped model of tests/test_seqlen.py
    (two GRU layers, H = 64, T = 7, a 12-entry ring; accounts with 0, 1, 3, ring - 1 and ring events and
    an unknown id): AbuseGpu derives each window from ev_count and gives the scores of the CPU engine -
    the executor on the left-aligned histories - within the f32-faithful kernels' bound. The packs take
    no cluster path; the native abuse device adds no cluster buckets and answers the same."""
    from igaming_platform_amd.engine.acct import AbuseNativeDevice
    from igaming_platform_amd.native import native
    from igaming_platform_amd.proto import risk_v1 as P
    from tests.test_acct import _ask
    from tests.test_seqlen import NOW, SVC_T, svc_engine, svc_expected, svc_model
    want, plain, lens = svc_expected()
    c, ids = svc_engine("cpu", svc_model())
    cpu = np.array([r.model_score for r in c.check_bonus_abuse_batch(ids, now=NOW)[:-1]])
    c.close()
    g, _ = svc_engine("gpu", svc_model())
    ag = g.abuse.gpu[0]
    assert ag.gm.masked and ag.T == SVC_T and ag.gm.split
    assert not ag.gp.ws_ok and not ag.gp.wsx_ok and ag.gp.workspace(64) is None
    res = g.check_bonus_abuse_batch(ids, now=NOW)
    assert res[-1].model_score is None
    got = np.array([r.model_score for r in res[:-1]])
    gap = float(np.abs(got - cpu).max())
    print(f"masked abuse model gpu {got} vs cpu {cpu}: gap {gap:.2e}; unmasked twin {plain}")
    assert gap <= G.SPLIT_TOL and float(np.abs(got - want).max()) <= G.SPLIT_TOL
    assert np.all(np.abs(got - plain)[lens < SVC_T] > 1e-3)
    if g.acct is not None:
        devs = [d for d in g.acct.devices if isinstance(d, AbuseNativeDevice)]
        assert devs and all(d.buckets == [64] and d.gm.masked for d in devs)
        reqs = [(native().RPC_ABUSE, P.CheckBonusAbuseRequest(account_id=a, bonus_id="welcome")) for a in ids]
        for r, (b, e) in zip(res[:-1], _ask(g.acct.router, reqs, now=NOW)):
            assert e is None and abs(P.CheckBonusAbuseResponse.FromString(b).abuse_score - r.abuse_score) <= 1e-6
    g.close()
