"""Cases, operands and float64 references for the K4 edge tests (tests/test_gru_edges.py without a
GPU, tests/test_gru_edges_gpu.py on the device): the GRU kernels of gru.hip (gru_kernel,
gru2_pipe_kernel, gru_x3_kernel), gru_ws.hip and gru_wsx.hip on every dispatch path, at T = 1, 2, 3,
with live counts that end inside a workgroup or a cluster, X wider than the launch, event rings
longer than T and the reverse direction.

Weights follow onnx/builders.py (uniform +-1 / sqrt(H)); the head weight is scaled x40 so the
sigmoid scores spread over (0, 1) instead of sitting at 0.5. X ~ N(0, 1), fixed seeds."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.dense_cases import SENTINEL, bf16r

HEAD_SCALE = 40.0
X_ALLOC = 132   # rows of every generated X (the cluster cases reach 129)
BP_ROWS = 47    # batch-parallel launches: 47 rows ...
BP_XROWS = 50   # ... inside an X of 50 rows
# (n_rows, live count through m_ptr): none; one live row in the last workgroup at either tile size;
# whole workgroups with no live row; one row
BP_LIVE = [(BP_ROWS, None), (BP_ROWS, 33), (BP_ROWS, 16), (1, None)]

# The bf16 tolerances are measured on the reference alone (test_gru_edges.py
# test_tolerances_come_from_the_reference): the bf16 emulation below in float32 against the same in
# float64, over every (model, direction, input) of the tables; the largest difference is the noise of
# bf16 rounding flips that any correct f32 implementation shares. Each tolerance is 4x that maximum
# (the 4x covers the kernels' __expf and MFMA accumulation order).
# Measured maxima: yh 1.14e-4 (G, 12 steps at K = 64 + 256), out 4.67e-4 (E from the event rings, 100 steps).
YH_TOL = 4.6e-4
OUT_TOL = 1.9e-3
SPLIT_TOL = 1e-4   # f32-faithful kernels against float64 (test_gru_split_mode_fp32_faithful_over_100_steps)
HEAD_ORDER_TOL = 1e-6  # out of two bf16 paths with bit-equal yh: only the head's cross-wave sum order differs

Model = namedtuple("Model", "name H layers lbr I T seed")

# the issue's eight models
TABLE = [
    Model("A", 64, 1, 1, 8, 1, 101),
    Model("B", 64, 2, 0, 24, 2, 102),
    Model("C", 128, 2, 1, 40, 3, 103),
    Model("D", 128, 1, 0, 64, 5, 104),
    Model("E", 256, 2, 1, 16, 7, 105),
    Model("F", 256, 2, 0, 32, 4, 106),
    Model("G", 256, 2, 1, 64, 12, 107),
    Model("H", 256, 1, 1, 8, 9, 108),
]
# E at 1- and 4-chunk staging and at T = 1, 2, 3 (the cluster kernels' parity buffers, the pipelined
# kernel's prologue / epilogue at H = 256)
E_VARIANTS = [
    Model("E8", 256, 2, 1, 8, 7, 105),
    Model("E32", 256, 2, 1, 32, 7, 105),
    Model("E_T1", 256, 2, 1, 16, 1, 105),
    Model("E_T2", 256, 2, 1, 16, 2, 105),
    Model("E_T3", 256, 2, 1, 16, 3, 105),
]
# two-layer models at the (H, K padding of the input, lbr) combinations the table leaves out, so that
# every gru_kernel / gru2_pipe_kernel / gru_x3_kernel instance launch_gru can pick is launched
FILL = [
    Model("A2", 64, 2, 1, 8, 3, 111),
    Model("B40", 64, 2, 0, 40, 1, 112),
    Model("A2_48", 64, 2, 1, 48, 2, 113),
    Model("C16", 128, 2, 1, 16, 2, 114),
    Model("D2_24", 128, 2, 0, 24, 3, 115),
    Model("D2", 128, 2, 0, 64, 1, 116),
    Model("F40", 256, 2, 0, 40, 2, 117),
]
MODELS = {m.name: m for m in TABLE + E_VARIANTS + FILL}
CLUSTER_MODELS = ["E", "E8", "E32", "E_T1", "E_T2", "E_T3"]
REVERSE_MODELS = ["B", "E"]

# cluster kernels: (launch rows, live count through m_ptr); the last of each ends inside a cluster
CLUSTER_ROWS = {
    1: [(1, None), (127, None), (129, None), (129, 100)],          # gru_ws_kernel<false>, 128-row clusters
    2: [(1, None), (127, None), (129, None), (129, 100)],          # gru_ws_kernel<true>
    3: [(1, None), (63, None), (65, None), (129, None), (129, 100)],  # gru_ws2_kernel, 64-row
    "wsx": [(1, None), (31, None), (33, None), (65, None), (65, 40)],  # gru_wsx_kernel, 32-row
}
CLUSTER_KERNEL = {1: "gru_ws_kernel<false>", 2: "gru_ws_kernel<true>", 3: "gru_ws2_kernel", "wsx": "gru_wsx_kernel"}

# event rings (model E, I = 16 = the default event width): T below the ring and T = ring
RING_ROWS = 48
RING_T = [7, "ring"]


# ------------------------------------------------------------------------------ operands
@lru_cache(maxsize=None)
def weights(name):
    """(layers, head): layers = [(W [3H, I], R [3H, H], B [6H], lbr), ...] float32 in ONNX gate order
    z, r, h (B = Wb | Rb); head = (w [H], b, "sigmoid")."""
    m = MODELS[name]
    rng = np.random.default_rng(m.seed)
    s = 1.0 / np.sqrt(m.H)
    layers = []
    # the recurrent and bias draws come first, so that E8 / E32 / E_T* share E's R, B and head
    rb = [(rng.uniform(-s, s, (3 * m.H, m.H)).astype(np.float32), rng.uniform(-s, s, 6 * m.H).astype(np.float32))
          for _ in range(m.layers)]
    wh = (rng.standard_normal(m.H) * np.sqrt(1.0 / m.H) * HEAD_SCALE).astype(np.float32)
    for i in range(m.layers):
        k = m.I if i == 0 else m.H
        layers.append((rng.uniform(-s, s, (3 * m.H, k)).astype(np.float32), rb[i][0], rb[i][1], m.lbr))
    return layers, (wh, 0.125, "sigmoid")


@lru_cache(maxsize=None)
def dense_x(name):
    """X [T, X_ALLOC, I] float32."""
    m = MODELS[name]
    return np.random.default_rng(m.seed + 1000).standard_normal((m.T, X_ALLOC, m.I)).astype(np.float32)


def nan_past(X, live, x_rows):
    """X[:, :x_rows] with every row at and past ``live`` NaN: a kernel that reads one turns NaN."""
    X = np.array(X[:, :x_rows])
    X[:, live:] = np.nan
    return X


def plan_steps(name):
    """The model as models.plan steps (what GruPack takes): ([GRUStep, ...], DenseStep head)."""
    from igaming_platform_amd.models.plan import DenseStep, GRUStep
    m = MODELS[name]
    layers, (wh, bh, act) = weights(name)
    gs = [GRUStep(m.H, W.shape[1], lbr, W, R, B, seq=m.T) for W, R, B, lbr in layers]
    return gs, DenseStep(1, m.H, act, wh[None, :], np.array([bh], np.float32))


def onnx_gru(name, T, reverse=False, head=True):
    """Serialized ONNX twin: GRU [-> Squeeze -> GRU] -> Y_h [-> Gemm -> Sigmoid]."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    m = MODELS[name]
    layers, (wh, bh, _) = weights(name)
    attrs = dict(hidden_size=m.H, linear_before_reset=m.lbr)
    if reverse:
        attrs["direction"] = "reverse"
    inits = [tensor("ax1", np.array([1], np.int64)), tensor("shp", np.array([-1, m.H], np.int64))]
    nodes, cur = [], "input"
    for i, (W, R, B, _) in enumerate(layers):
        if i:
            nodes.append(node("Squeeze", [f"Y{i - 1}", "ax1"], [f"X{i}"]))
            cur = f"X{i}"
        nodes.append(node("GRU", [cur, f"W{i}", f"R{i}", f"B{i}"], [f"Y{i}", f"Yh{i}"], **attrs))
        inits += [tensor(f"W{i}", W[None]), tensor(f"R{i}", R[None]), tensor(f"B{i}", B[None])]
    last = f"Yh{len(layers) - 1}"
    if head:
        nodes += [node("Reshape", [last, "shp"], ["h"]), node("Gemm", ["h", "Wh", "Bh"], ["logit"]),
                  node("Sigmoid", ["logit"], ["output"])]
        inits += [tensor("Wh", np.ascontiguousarray(wh[:, None])), tensor("Bh", np.array([bh], np.float32))]
        out = value_info("output", S.FLOAT, ["N", 1])
    else:
        nodes.append(node("Reshape", [last, "shp"], ["output"]))
        out = value_info("output", S.FLOAT, ["N", m.H])
    return model(nodes, [value_info("input", S.FLOAT, [T, "N", m.I])], [out], inits, name="gru_edges",
                 metadata={"family": "gru"}).SerializeToString()


# ------------------------------------------------------------------------------ reference
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def bf16_rne(a):
    """``a`` (finite) rounded to float32, then to bfloat16 to nearest even, in integer arithmetic
    (dense_cases.bf16r without the trip through torch); float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def gru_ref(layers, head, X, *, reverse=False, bf16=False, dtype=np.float64, probe=None):
    """(yh [rows, H], out [rows] | None) of the GRU stack over X [T, rows, I], plain numpy in ``dtype``.
    ``bf16``: rounds (to nearest even) exactly where gru.hip layer_step does - x_t, W and R, the
    h_{t-1} operand of the recurrent product, r * h when linear_before_reset = 0, and layer 2's input
    (layer 1's rounded h); the carried state, gates, biases and head stay unrounded. ``dtype``
    float32 runs the same emulation in single precision (the tolerance measurement).
    ``probe``: a wrong kernel, for the tolerance conditions - ("unit", j) drops hidden unit j before
    the head, ("bias", j) zeroes the last layer's Rb_h of unit j, ("column",) ignores the last input
    column."""
    def rnd(a):
        return bf16_rne(a).astype(dtype) if bf16 else np.asarray(a, dtype)
    x = np.asarray(X, dtype)
    if probe and probe[0] == "column":
        x = x.copy()
        x[:, :, -1] = 0
    if reverse:
        x = x[::-1]
    x = rnd(x)
    T, rows = x.shape[:2]
    for li, (W, R, B, lbr) in enumerate(layers):
        H = R.shape[1]
        Wq, Rq, B = rnd(W), rnd(R), np.array(B, dtype)
        if probe and probe[0] == "bias" and li == len(layers) - 1:
            B[5 * H + probe[1]] = 0
        Wb, Rb = B[:3 * H], B[3 * H:]
        h = np.zeros((rows, H), dtype)
        ys = []
        for t in range(T):
            hq = rnd(h)
            xw = x[t] @ Wq.T
            z = _sig(xw[:, :H] + hq @ Rq[:H].T + Wb[:H] + Rb[:H])
            r = _sig(xw[:, H:2 * H] + hq @ Rq[H:2 * H].T + Wb[H:2 * H] + Rb[H:2 * H])
            if lbr:
                hh = np.tanh(xw[:, 2 * H:] + Wb[2 * H:] + r * (hq @ Rq[2 * H:].T + Rb[2 * H:]))
            else:
                hh = np.tanh(xw[:, 2 * H:] + Wb[2 * H:] + rnd(r * h) @ Rq[2 * H:].T + Rb[2 * H:])
            h = (1 - z) * hh + z * h
            ys.append(h)
        x = rnd(np.stack(ys))
    yh, out = h, None
    if head is not None:
        w, b, act = head
        hv = yh
        if probe and probe[0] == "unit":
            hv = yh.copy()
            hv[:, probe[1]] = 0
        out = hv @ np.asarray(w, dtype) + dtype(b)
        if act == "sigmoid":
            out = _sig(out)
    return yh, out


def probes(name):
    """The three wrong kernels of condition (b), at the units with the median |head weight| and the
    median |Rb_h| of the last layer (a typical unit, not the one that shows best)."""
    layers, (wh, _, _) = weights(name)
    H = MODELS[name].H
    med = lambda v: int(np.argsort(np.abs(v))[len(v) // 2])
    return [("unit", med(wh)), ("bias", med(layers[-1][2][5 * H:])), ("column",)]


# ------------------------------------------------------------------------------ event rings
def ring_gather(ev, ev_head, ev_count, slots, T):
    """Host gather of the kernels' event-ring input: X [T, rows, D] from ev [C, ring, D], right-aligned,
    oldest event first - the last T ring entries before ``ev_head``, min(ev_count, T) of them live;
    zeros before the first event and for slot -1."""
    C, ring, D = ev.shape
    X = np.zeros((T, len(slots), D), np.float32)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        cnt, head = min(int(ev_count[s]), T), int(ev_head[s])
        for t in range(T - cnt, T):
            X[t, b] = ev[s, (head - T + t) % ring]
    return X


@lru_cache(maxsize=None)
def ring_case(ring, D, T):
    """(ev [C, ring, D] bf16-exact float32, ev_head [C], ev_count [C], slots [RING_ROWS]): every
    (ev_count, ev_head) of {0, 1, T-1, T, T+1, ring} x {0, 1, ring-1}, some slots -1."""
    counts = [0, 1, T - 1, T, min(T + 1, ring), ring]
    heads = [0, 1, ring - 1]
    combos = [(c, h) for c in counts for h in heads]
    C = len(combos) + 6
    rng = np.random.default_rng(900 + T)
    ev = bf16r(rng.standard_normal((C, ring, D))).astype(np.float32)
    ev_head = np.array([h for _, h in combos] + list(rng.integers(0, ring, 6)), np.int32)
    ev_count = np.array([c for c, _ in combos] + list(rng.integers(0, ring + 1, 6)), np.int32)
    slots = (np.arange(RING_ROWS) % C).astype(np.int32)
    slots[len(combos)::5] = -1
    return ev, ev_head, ev_count, slots


def default_ring():
    """(ring length, event width) of the default feature configuration."""
    from igaming_platform_amd.config import FeatureConfig
    fc = FeatureConfig()
    return fc.event_ring, fc.event_dim


@lru_cache(maxsize=None)
def ring_x(T):
    """The event-ring case of ``T`` (an entry of RING_T) gathered on the host: (T, X [T, RING_ROWS, D])."""
    ring, D = default_ring()
    T = ring if T == "ring" else T
    ev, head, count, slots = ring_case(ring, D, T)
    return T, ring_gather(ev, head, count, slots, T)


def ref_inputs():
    """Every (label, model, X, reverse) the device tests compare with a reference."""
    for name in MODELS:
        yield f"{name}-dense", name, dense_x(name), False
    for name in REVERSE_MODELS:
        yield f"{name}-dense-reverse", name, dense_x(name), True
    for T in RING_T:
        for rev in (False, True):
            yield f"E-ring-{T}" + ("-reverse" if rev else ""), "E", ring_x(T)[1], rev


@lru_cache(maxsize=None)
def reference(label, bf16):
    """(yh, out) float64 of the labelled reference input, computed once."""
    for lab, name, X, rev in ref_inputs():
        if lab == label:
            layers, head = weights(name)
            return gru_ref(layers, head, X, reverse=rev, bf16=bf16)
    raise KeyError(label)


# ------------------------------------------------------------------------------ dispatch mirror
def _x3_lds(RT, KSX, KSH, NW, lbr):
    M, H = RT * 16, KSH * 32
    HS, XS = H + 8, KSX * 32 + 8
    return 8 * M * HS * 2 + 4 * M * XS * 2 + (0 if lbr else 2 * M * HS * 2) + 2 * 6 * H * 4 + NW * M * 4


def dispatch(m, *, rows, tile_rows=0, pipeline=1, waves=0, ws=0, split=False, n_cu=256):
    """What launch_gru (gru.hip) launches for model ``m``: (kernel, RT, KSX, KSH, LBR, NW) for the
    batch-parallel kernels, (kernel,) for the cluster kernels."""
    KSX, KSH = (1 if m.I <= 32 else 2), m.H // 32
    cluster_shape = m.layers == 2 and m.H == 256 and m.lbr == 1 and m.I <= 32
    if split:
        if ws and cluster_shape and -(-rows // 32) * 16 <= n_cu // 2:
            return ("gru_wsx_kernel",)
        NW = 8 if KSH >= 4 else 4
        if KSH == 8 and waves != 8 and m.lbr:
            rt = 2 if tile_rows == 32 else 1
            if rt == 1 or _x3_lds(2, KSX, KSH, 16, 1) <= 160 * 1024:
                return ("gru_x3_kernel", rt, KSX, KSH, 1, 16)
        if m.lbr and tile_rows == 32 and _x3_lds(2, KSX, KSH, NW, 1) <= 160 * 1024:
            return ("gru_x3_kernel", 2, KSX, KSH, 1, NW)
        return ("gru_x3_kernel", 1, KSX, KSH, m.lbr, NW)
    if ws and cluster_shape:
        if ws == 3 and -(-rows // 64) * 8 <= 2 * n_cu:
            return ("gru_ws2_kernel",)
        if ws != 3 and -(-rows // 128) * 8 <= n_cu:
            return ("gru_ws_kernel<true>" if ws == 2 else "gru_ws_kernel<false>",)
    tr = tile_rows or (32 if rows >= 32 * 256 else 16)
    RT = 2 if tr == 32 else 1
    if m.layers == 2 and pipeline:
        return ("gru2_pipe_kernel", RT, KSX, KSH, m.lbr, {8: 16, 4: 8, 2: 4}[KSH])
    NW = 8 if KSH >= 4 and waves != 4 else 4
    return ("gru_kernel", RT, KSX, KSH, m.lbr, NW)


def bf16_paths(name):
    """[(launch options, instance)] of the model's bf16 batch-parallel paths, the anchor (tile 16,
    pipelined when two layers, default waves) first; one entry per distinct instance."""
    m = MODELS[name]
    seen, out = set(), []
    for pipeline in ((1, 0) if m.layers == 2 else (1,)):
        for waves in ((0, 4) if m.H >= 128 else (0,)):
            for tile in (16, 32):
                inst = dispatch(m, rows=BP_ROWS, tile_rows=tile, pipeline=pipeline, waves=waves)
                if inst not in seen:
                    seen.add(inst)
                    out.append((dict(tile_rows=tile, pipeline=pipeline, waves=waves), inst))
    return out


def split_paths(name):
    """[(launch options, instance)] of the model's f32-faithful batch-parallel paths."""
    m = MODELS[name]
    seen, out = set(), []
    for waves in ((0, 8) if m.H == 256 else (0,)):
        for tile in (16, 32):
            inst = dispatch(m, rows=BP_ROWS, tile_rows=tile, waves=waves, split=True)
            if inst not in seen:
                seen.add(inst)
                out.append((dict(tile_rows=tile, waves=waves), inst))
    return out


# bf16 instances that are not bit-equal to their model's anchor on the device, with the measured gap:
# held to the reference tolerance instead (none: every pair measured bit-equal)
NOT_BIT_EQUAL = {}


# ------------------------------------------------------------------------------ comparison
def compare(yh, out, ref_yh, ref_out, live, yh_tol, out_tol, what=""):
    """The device test's check of one launch: ``yh`` [alloc, H] / ``out`` [alloc] float32 arrays that
    were pre-filled with SENTINEL. Rows below ``live`` hold no NaN and lie within the tolerances of
    the reference rows; every row at and past ``live`` still is the sentinel, bit for bit. No row
    and no model is left out. Returns the gaps (yh, out)."""
    yh, out = np.asarray(yh), np.asarray(out)
    sent = np.float32(SENTINEL).view(np.int32)
    assert np.all(yh[live:].view(np.int32) == sent), f"{what}: yh written past the live rows"
    assert np.all(out[live:].view(np.int32) == sent), f"{what}: out written past the live rows"
    assert not np.isnan(yh[:live]).any() and not np.isnan(out[:live]).any(), f"{what}: NaN"
    g_yh = float(np.abs(yh[:live].astype(np.float64) - ref_yh[:live]).max())
    g_out = float(np.abs(out[:live].astype(np.float64) - ref_out[:live]).max())
    assert g_yh <= yh_tol, f"{what}: yh off by {g_yh:.3e} > {yh_tol:.1e}"
    assert g_out <= out_tol, f"{what}: out off by {g_out:.3e} > {out_tol:.1e}"
    return g_yh, g_out
