"""Cases, operands and float64 references for the K4 LSTM edge tests (tests/test_lstm_edges.py
without a GPU, tests/test_lstm_edges_gpu.py on the device): every lstm_kernel<RT, KSX, KSH, NW, SPLIT>
instance launch_lstm (lstm.hip) can pick, at T = 1, 2, 3, with 1 to 8 eight-element chunks per input
row, live counts that end inside a 32-row tile, X wider than the launch, event rings and the reverse
direction.

Weights follow onnx/builders.py (uniform +-1 / sqrt(H)); the head weight is scaled x100 so the sigmoid
scores spread over (0, 1) instead of sitting at 0.5. LSTM states are smaller than GRU states (rms h
0.013 for E at T = 1), so the GRU suite's x40 leaves E_T1 a spread of 0.14, below condition (c) of
test_lstm_edges.py; at x100 every reference input spans at least 0.33 (E_T1). The bias-driven mean of
h puts a constant w . mean(h) into every logit, which at this scale saturates the scores of some
draws: the seeds of C, E and F are ones where it does not. X ~ N(0, 1), fixed seeds."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.dense_cases import SENTINEL, bf16r
from tests.gru_cases import bf16_rne

HEAD_SCALE = 100.0
HEAD_BIAS = 0.125
BP_ROWS = 47    # batch-parallel launches: 47 rows ...
BP_XROWS = 50   # ... inside an X of 50 rows
# (n_rows, live count through m_ptr): none; one live row in the last workgroup at either tile size;
# whole workgroups with no live row; nothing live (nothing is written); one row
BP_LIVE = [(BP_ROWS, None), (BP_ROWS, 33), (BP_ROWS, 16), (BP_ROWS, 0), (1, None)]

# The bf16 tolerances are measured on the reference alone (test_lstm_edges.py
# test_tolerances_come_from_the_reference): the bf16 emulation below in float32 against the same in
# float64, over every (model, direction, input) of the tables; the largest difference is the noise of
# bf16 rounding flips that any correct f32 implementation shares. Each tolerance is 4x that maximum
# (the 4x covers the kernel's __expf and MFMA accumulation order, as for the GRU).
# Measured maxima: yh 4.65e-5 and out 7.51e-4 (both B56, 3 steps at K = 64 + 64), the logit of A
# without its sigmoid 2.55e-6.
YH_TOL = 1.87e-4
OUT_TOL = 3.01e-3
LOGIT_TOL = 1.02e-5   # A's head without the sigmoid (the sigmoid's slope is at most 1 / 4)
SPLIT_TOL = 1e-4  # f32-faithful kernels against float64 (test_lstm_split_mode_fp32_faithful_over_100_steps)
EXECUTOR_TOL = 2e-6  # the float64 reference against the fp32 C++ executor (test_lstm_gpu.py's _lstm_f64 check)

Model = namedtuple("Model", "name H layers I T seed act")

TABLE = [
    Model("A", 64, 1, 8, 1, 201, "sigmoid"),
    Model("B", 64, 2, 40, 2, 202, "sigmoid"),
    Model("C", 128, 2, 24, 3, 307, "sigmoid"),
    Model("D", 128, 1, 64, 5, 204, "sigmoid"),
    Model("E", 256, 2, 16, 7, 317, "sigmoid"),
    Model("F", 256, 2, 64, 4, 304, "sigmoid"),
    Model("G", 256, 1, 48, 12, 207, "sigmoid"),
    Model("H", 64, 2, 32, 9, 208, "sigmoid"),
    # E's weights (same seed and shapes) at T = 1, 2, 3: the t + 1 prefetch, the ping-pong parity and
    # the t + 1 < T store guard at the widest H
    Model("E_T1", 256, 2, 16, 1, 317, "sigmoid"),
    Model("E_T2", 256, 2, 16, 2, 317, "sigmoid"),
    Model("E_T3", 256, 2, 16, 3, 317, "sigmoid"),
    Model("B56", 64, 2, 56, 3, 209, "sigmoid"),
    # A's weights with the head's activation left out
    Model("A_none", 64, 1, 8, 1, 201, "none"),
]
MODELS = {m.name: m for m in TABLE}
REVERSE_MODELS = ["B", "E"]

# one bidirectional layer through the runner (LstmModel): (name, H, I, T, seed)
BiModel = namedtuple("BiModel", "name H I T seed")
BI_MODELS = {m.name: m for m in [BiModel("BI64", 64, 40, 3, 221), BiModel("BI256", 256, 16, 3, 222)]}
BI_ROWS = [1, BP_ROWS]

# event rings (model E, I = 16 = the default event width): a 12-entry ring, T below it and T = ring
RING = 12
RING_ROWS = 48
RING_T = [7, RING]


def tol(name):
    """(yh, out) bf16 tolerances of a model."""
    return YH_TOL, (LOGIT_TOL if MODELS[name].act == "none" else OUT_TOL)


# ------------------------------------------------------------------------------ operands
def _layer(rng, H, k):
    s = 1.0 / np.sqrt(H)
    return (rng.uniform(-s, s, (4 * H, k)).astype(np.float32), rng.uniform(-s, s, (4 * H, H)).astype(np.float32),
            rng.uniform(-s, s, 8 * H).astype(np.float32))


@lru_cache(maxsize=None)
def weights(name):
    """(layers, head): layers = [(W [4H, I], R [4H, H], B [8H]), ...] float32 in ONNX gate order
    i, o, f, c (B = Wb | Rb); head = (w [H], b, act)."""
    m = MODELS[name]
    rng = np.random.default_rng(m.seed)
    layers = [_layer(rng, m.H, m.I if i == 0 else m.H) for i in range(m.layers)]
    wh = (rng.standard_normal(m.H) * np.sqrt(1.0 / m.H) * HEAD_SCALE).astype(np.float32)
    return layers, (wh, HEAD_BIAS, m.act)


@lru_cache(maxsize=None)
def bi_weights(name):
    """(forward layer, reverse layer, head over 2H) of a bidirectional model."""
    m = BI_MODELS[name]
    rng = np.random.default_rng(m.seed)
    fwd, rev = _layer(rng, m.H, m.I), _layer(rng, m.H, m.I)
    wh = (rng.standard_normal(2 * m.H) * np.sqrt(0.5 / m.H) * HEAD_SCALE).astype(np.float32)
    return fwd, rev, (wh, HEAD_BIAS, "sigmoid")


@lru_cache(maxsize=None)
def dense_x(name):
    """X [T, BP_XROWS, I] float32."""
    m = MODELS.get(name) or BI_MODELS[name]
    X = np.random.default_rng(m.seed + 1000).standard_normal((m.T, BP_XROWS, m.I)).astype(np.float32)
    X.setflags(write=False)
    return X


def nan_past(X, live):
    """A copy of X with every row at and past ``live`` NaN: a kernel that reads one turns NaN."""
    X = np.array(X)
    X[:, live:] = np.nan
    return X


def plan_steps(name):
    """The model as models.plan steps (what LstmPack takes): ([LSTMStep, ...], DenseStep head)."""
    from igaming_platform_amd.models.plan import DenseStep, LSTMStep
    m = MODELS[name]
    layers, (wh, bh, act) = weights(name)
    ls = [LSTMStep(m.H, W.shape[1], W, R, B, seq=m.T) for W, R, B in layers]
    return ls, DenseStep(1, m.H, act, wh[None, :], np.array([bh], np.float32))


def onnx_lstm(name, T, reverse=False, head=True):
    """Serialized ONNX twin: LSTM [-> Squeeze -> LSTM] -> Y_h [-> Gemm [-> Sigmoid]]."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    m = MODELS[name]
    layers, (wh, bh, act) = weights(name)
    attrs = dict(hidden_size=m.H)
    if reverse:
        attrs["direction"] = "reverse"
    inits = [tensor("ax1", np.array([1], np.int64)), tensor("shp", np.array([-1, m.H], np.int64))]
    nodes, cur = [], "input"
    for i, (W, R, B) in enumerate(layers):
        if i:
            nodes.append(node("Squeeze", [f"Y{i - 1}", "ax1"], [f"X{i}"]))
            cur = f"X{i}"
        nodes.append(node("LSTM", [cur, f"W{i}", f"R{i}", f"B{i}"], [f"Y{i}", f"Yh{i}"], **attrs))
        inits += [tensor(f"W{i}", W[None]), tensor(f"R{i}", R[None]), tensor(f"B{i}", B[None])]
    last = f"Yh{len(layers) - 1}"
    if head:
        nodes += [node("Reshape", [last, "shp"], ["h"]),
                  node("Gemm", ["h", "Wh", "Bh"], ["logit" if act == "sigmoid" else "output"])]
        if act == "sigmoid":
            nodes.append(node("Sigmoid", ["logit"], ["output"]))
        inits += [tensor("Wh", np.ascontiguousarray(wh[:, None])), tensor("Bh", np.array([bh], np.float32))]
        out = value_info("output", S.FLOAT, ["N", 1])
    else:
        nodes.append(node("Reshape", [last, "shp"], ["output"]))
        out = value_info("output", S.FLOAT, ["N", m.H])
    return model(nodes, [value_info("input", S.FLOAT, [T, "N", m.I])], [out], inits, name="lstm_edges",
                 metadata={"family": "lstm"}).SerializeToString()


def onnx_bilstm(name, head=True):
    """Serialized ONNX twin of a bidirectional model: LSTM -> Y_h [2, N, H] -> Transpose -> [N, 2H]
    [-> Gemm -> Sigmoid], the graph onnx/builders.py writes."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    m = BI_MODELS[name]
    fwd, rev, (wh, bh, _) = bi_weights(name)
    nodes = [node("LSTM", ["input", "W", "R", "B"], ["Y", "Yh"], hidden_size=m.H, direction="bidirectional"),
             node("Transpose", ["Yh"], ["hT"], perm=[1, 0, 2])]
    inits = [tensor(k, np.stack([a, b])) for k, a, b in zip("WRB", fwd, rev)]
    inits.append(tensor("shp", np.array([-1, 2 * m.H], np.int64)))
    if head:
        nodes += [node("Reshape", ["hT", "shp"], ["h"]), node("Gemm", ["h", "Wh", "Bh"], ["logit"]),
                  node("Sigmoid", ["logit"], ["output"])]
        inits += [tensor("Wh", np.ascontiguousarray(wh[:, None])), tensor("Bh", np.array([bh], np.float32))]
        out = value_info("output", S.FLOAT, ["N", 1])
    else:
        nodes.append(node("Reshape", ["hT", "shp"], ["output"]))
        out = value_info("output", S.FLOAT, ["N", 2 * m.H])
    return model(nodes, [value_info("input", S.FLOAT, [m.T, "N", m.I])], [out], inits, name="lstm_edges_bi",
                 metadata={"family": "lstm"}).SerializeToString()


# ------------------------------------------------------------------------------ reference
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_ref(layers, head, X, *, reverse=False, bf16=False, dtype=np.float64, probe=None):
    """(yh [rows, H], out [rows] | None) of the LSTM stack over X [T, rows, I], plain numpy in
    ``dtype``. Gate order i, o, f, c; states start at zero; the bias is Wb + Rb, summed in float32 as
    the kernel does. ``bf16``: rounds (to nearest even) exactly where lstm_kernel<..., 0> does - x_t,
    W and R, and the h that is stored to LDS (the recurrent operand of the next step and layer 2's
    input); c, the carried h that reaches yh and the head, the gates, biases and head stay unrounded.
    ``dtype`` float32 runs the same emulation in single precision (the tolerance measurement).
    ``probe``: a wrong kernel, for the tolerance conditions - ("unit", j) drops hidden unit j before
    the head, ("bias",) ignores the last layer's Rb, ("column",) ignores the last input column."""
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
    for li, (W, R, B) in enumerate(layers):
        H = R.shape[1]
        Wq, Rq, B = rnd(W), rnd(R), np.asarray(B, np.float32)
        bias = B[:4 * H] + B[4 * H:]
        if probe and probe[0] == "bias" and li == len(layers) - 1:
            bias = B[:4 * H]
        bias = bias.astype(dtype)
        h = np.zeros((rows, H), dtype)
        c = np.zeros((rows, H), dtype)
        ys = []
        for t in range(T):
            a = x[t] @ Wq.T + rnd(h) @ Rq.T + bias
            i, o, f = _sig(a[:, :H]), _sig(a[:, H:2 * H]), _sig(a[:, 2 * H:3 * H])
            c = f * c + i * np.tanh(a[:, 3 * H:])
            h = o * np.tanh(c)
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


def bi_ref(name, X, head=True):
    """float64 (Y_h [rows, 2H] in the ONNX [N, 2, H] order, out [rows] | None) of a bidirectional model."""
    fwd, rev, (wh, bh, _) = bi_weights(name)
    yf, _ = lstm_ref([fwd], None, X)
    yr, _ = lstm_ref([rev], None, X, reverse=True)
    yh = np.concatenate([yf, yr], 1)
    return yh, (_sig(yh @ wh.astype(np.float64) + bh) if head else None)


def probes(name):
    """The three wrong kernels of condition (b); the dropped unit is the one with the median
    |head weight| (a typical unit, not the one that shows best)."""
    wh = weights(name)[1][0]
    return [("unit", int(np.argsort(np.abs(wh))[len(wh) // 2])), ("bias",), ("column",)]


# ------------------------------------------------------------------------------ event rings
def ring_gather(ev, ev_head, ev_count, slots, T):
    """Host gather of the kernel's event-ring input: X [T, rows, D] from ev [C, ring, D], right-aligned,
    oldest event first - the last T ring entries before ``ev_head``, min(ev_count, T) of them live;
    zeros before the first event and for slot -1. (In reverse mode the kernel walks this sequence
    last step first.)"""
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
def ring_case(T, D=16):
    """(ev [C, RING, D] bf16-exact float32, ev_head [C], ev_count [C], slots [RING_ROWS]): every
    (ev_count, ev_head) of {0, 3, T, RING} x {0, 3, RING - 1} (a head below the count has wrapped
    round the ring), six random accounts, slots that repeat and some that are -1."""
    combos = [(c, h) for c in sorted({0, 3, T, RING}) for h in (0, 3, RING - 1)]
    C = len(combos) + 6
    rng = np.random.default_rng(950 + T)
    ev = bf16r(rng.standard_normal((C, RING, D))).astype(np.float32)
    ev_head = np.array([h for _, h in combos] + list(rng.integers(0, RING, 6)), np.int32)
    ev_count = np.array([c for c, _ in combos] + list(rng.integers(0, RING + 1, 6)), np.int32)
    slots = (np.arange(RING_ROWS) % C).astype(np.int32)
    slots[C + 1::5] = -1
    return ev, ev_head, ev_count, slots


@lru_cache(maxsize=None)
def ring_x(T):
    """The event-ring case of ``T`` gathered on the host: X [T, RING_ROWS, D]."""
    ev, head, count, slots = ring_case(T)
    return ring_gather(ev, head, count, slots, T)


def ring_empty_rows(T):
    """Rows of the ring case with an empty history (no slot, or an account without events)."""
    _, _, count, slots = ring_case(T)
    return [b for b, s in enumerate(slots) if s < 0 or count[s] == 0]


def ref_inputs():
    """Every (label, model, X, reverse) the device tests compare with a reference."""
    for name in MODELS:
        yield f"{name}-dense", name, dense_x(name), False
    for name in REVERSE_MODELS:
        yield f"{name}-dense-reverse", name, dense_x(name), True
    for T in RING_T:
        for rev in (False, True):
            yield f"E-ring-{T}" + ("-reverse" if rev else ""), "E", ring_x(T), rev


@lru_cache(maxsize=None)
def reference(label, bf16):
    """(yh, out) float64 of the labelled reference input, computed once."""
    for lab, name, X, rev in ref_inputs():
        if lab == label:
            layers, head = weights(name)
            return lstm_ref(layers, head, X, reverse=rev, bf16=bf16)
    raise KeyError(label)


# ------------------------------------------------------------------------------ dispatch mirror
LDS_LIMIT = 160 * 1024


def lds_bytes(RT, KSX, KSH, NW, split):
    """lstm_lds_bytes: hb[halves][layer][pingpong][M][H + 8] | xb[halves][pingpong][M][KSX * 32 + 8]
    bf16, bias[2][4H] and red[NW][M] f32."""
    M, H = RT * 16, KSH * 32
    HS, XS, NH = H + 8, KSX * 32 + 8, 2 if split else 1
    return NH * (4 * M * HS + 2 * M * XS) * 2 + 2 * 4 * H * 4 + NW * M * 4


def dispatch(m, tile_rows=0, split=False):
    """The instance launch_lstm (lstm.hip) launches for model ``m``: (RT, KSX, KSH, NW, SPLIT).
    launch_lstm: KSH = H / 32; launch_lstm_h: KSX from the layer-1 input's padding (32 up to I = 32,
    else 64); launch_lstm_t: 8 waves from H = 128 up, else 4, and 32-row tiles only on request and
    only where their LDS image fits the 160 KiB."""
    KSX, KSH, SPLIT = (1 if m.I <= 32 else 2), m.H // 32, 1 if split else 0
    NW = 8 if KSH >= 4 else 4
    RT = 2 if tile_rows == 32 and lds_bytes(2, KSX, KSH, NW, SPLIT) <= LDS_LIMIT else 1
    return RT, KSX, KSH, NW, SPLIT


def paths(name, split):
    """[(launch options, instance)] of the model, one entry per distinct instance, the 16-row one first."""
    seen, out = set(), []
    for tile in (16, 32):
        inst = dispatch(MODELS[name], tile, split)
        if inst not in seen:
            seen.add(inst)
            out.append((dict(tile_rows=tile), inst))
    return out


# ------------------------------------------------------------------------------ comparison
def compare(yh, out, ref_yh, ref_out, live, yh_tol, out_tol, what=""):
    """The device test's check of one launch: ``yh`` [alloc, H] / ``out`` [alloc] float32 arrays that
    were pre-filled with SENTINEL. Rows below ``live`` hold no NaN and lie within the tolerances of
    the reference rows; every row at and past ``live`` still is the sentinel, bit for bit (live = 0:
    nothing was written). No row and no model is left out. Returns the gaps (yh, out)."""
    yh, out = np.asarray(yh), np.asarray(out)
    sent = np.float32(SENTINEL).view(np.int32)
    assert np.all(yh[live:].view(np.int32) == sent), f"{what}: yh written past the live rows"
    assert np.all(out[live:].view(np.int32) == sent), f"{what}: out written past the live rows"
    assert not np.isnan(yh[:live]).any() and not np.isnan(out[:live]).any(), f"{what}: NaN"
    g_yh = float(np.abs(yh[:live].astype(np.float64) - ref_yh[:live]).max(initial=0.0))
    g_out = float(np.abs(out[:live].astype(np.float64) - ref_out[:live]).max(initial=0.0))
    assert g_yh <= yh_tol, f"{what}: yh off by {g_yh:.3e} > {yh_tol:.1e}"
    assert g_out <= out_tol, f"{what}: out off by {g_out:.3e} > {out_tol:.1e}"
    return g_yh, g_out
