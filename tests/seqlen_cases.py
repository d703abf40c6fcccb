"""Cases and float64 references for per-sequence lengths (ONNX sequence_lens) in the K4 GRU and LSTM
kernels (tests/test_seqlen.py without a GPU, tests/test_seqlen_gpu.py on the device).

The reference needs no new recurrence: a row of length L is the unmasked float64 reference of
tests/gru_cases.py / tests/lstm_cases.py at T = L on that row's first L steps, and the zero state
through the head at L = 0. Weights come from those tables; X ~ N(0, 1) at this file's own seeds.

Lengths cycle through [0, 1, 2, T-1, T, 3, T, 1] from a per-case offset, so they differ inside
every 4-row accumulator group and inside every 16-row MFMA tile, and both extremes occur in the
first and in the last tile of the 47 rows."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests import gru_cases as G
from tests import lstm_cases as L

T = 7
ROWS = G.BP_ROWS      # 47 rows ...
XROWS = G.BP_XROWS    # ... inside an X of 50 rows
LIVE = [None, 33, 0]  # live counts through m_ptr: all 47, one that ends inside a tile, nothing live

# kind gru | lstm; model: a name of the kind's table; opts: the launch options of K.gru / K.lstm;
# inst: the instance the launch must reach, written out from launch_gru / launch_lstm -
# gru (kernel, RT, KSX, KSH, LBR, NW), lstm (RT, KSX, KSH, NW, SPLIT)
Case = namedtuple("Case", "id kind model T reverse split opts inst")


def _c(id, kind, model, inst, T=T, reverse=False, split=False, **opts):
    return Case(id, kind, model, T, reverse, split, opts, inst)


CASES = [
    # gru_kernel: LBR 1 and 0, 16- and 32-row tiles, 4 and 8 waves, one and two layers
    _c("gru-A", "gru", "A", ("gru_kernel", 1, 1, 2, 1, 4), tile_rows=16),
    _c("gru-A-32", "gru", "A", ("gru_kernel", 2, 1, 2, 1, 4), tile_rows=32),
    _c("gru-D", "gru", "D", ("gru_kernel", 1, 2, 4, 0, 8), tile_rows=16),
    _c("gru-D-w4", "gru", "D", ("gru_kernel", 1, 2, 4, 0, 4), tile_rows=16, waves=4),
    _c("gru-D-32", "gru", "D", ("gru_kernel", 2, 2, 4, 0, 8), tile_rows=32),
    _c("gru-B-unpiped", "gru", "B", ("gru_kernel", 1, 1, 2, 0, 4), tile_rows=16, pipeline=0),
    _c("gru-E-unpiped-32", "gru", "E", ("gru_kernel", 2, 1, 8, 1, 8), tile_rows=32, pipeline=0),
    # gru2_pipe_kernel at H = 64 and at H = 256 (16 waves), LBR 0 and 1, both tiles, reverse, T = 1, 2, 3
    _c("pipe-B", "gru", "B", ("gru2_pipe_kernel", 1, 1, 2, 0, 4), tile_rows=16),
    _c("pipe-B-reverse", "gru", "B", ("gru2_pipe_kernel", 1, 1, 2, 0, 4), reverse=True, tile_rows=16),
    _c("pipe-E", "gru", "E", ("gru2_pipe_kernel", 1, 1, 8, 1, 16), tile_rows=16),
    _c("pipe-E-32", "gru", "E", ("gru2_pipe_kernel", 2, 1, 8, 1, 16), tile_rows=32),
    _c("pipe-E-T1", "gru", "E", ("gru2_pipe_kernel", 1, 1, 8, 1, 16), T=1, tile_rows=16),
    _c("pipe-E-T2", "gru", "E", ("gru2_pipe_kernel", 1, 1, 8, 1, 16), T=2, tile_rows=16),
    _c("pipe-E-T3", "gru", "E", ("gru2_pipe_kernel", 1, 1, 8, 1, 16), T=3, tile_rows=16),
    _c("pipe-F", "gru", "F", ("gru2_pipe_kernel", 1, 1, 8, 0, 16), tile_rows=16),
    # gru_x3_kernel: LBR 1 and 0, both tiles, the H = 256 16-wave instances
    _c("x3-A", "gru", "A", ("gru_x3_kernel", 1, 1, 2, 1, 4), split=True, tile_rows=16),
    _c("x3-A-32", "gru", "A", ("gru_x3_kernel", 2, 1, 2, 1, 4), split=True, tile_rows=32),
    _c("x3-B", "gru", "B", ("gru_x3_kernel", 1, 1, 2, 0, 4), split=True, tile_rows=16),
    _c("x3-D", "gru", "D", ("gru_x3_kernel", 1, 2, 4, 0, 8), split=True, tile_rows=16),
    _c("x3-E", "gru", "E", ("gru_x3_kernel", 1, 1, 8, 1, 16), split=True, tile_rows=16),
    _c("x3-E-32", "gru", "E", ("gru_x3_kernel", 2, 1, 8, 1, 16), split=True, tile_rows=32),
    _c("x3-E-reverse", "gru", "E", ("gru_x3_kernel", 1, 1, 8, 1, 16), reverse=True, split=True, tile_rows=16),
    # lstm_kernel: SPLIT 0 and 1, both tiles, one and two layers, reverse
    _c("lstm-A", "lstm", "A", (1, 1, 2, 4, 0), tile_rows=16),
    _c("lstm-A-32", "lstm", "A", (2, 1, 2, 4, 0), tile_rows=32),
    _c("lstm-A-split", "lstm", "A", (1, 1, 2, 4, 1), split=True, tile_rows=16),
    _c("lstm-B-reverse", "lstm", "B", (1, 2, 2, 4, 0), reverse=True, tile_rows=16),
    _c("lstm-E", "lstm", "E", (1, 1, 8, 8, 0), tile_rows=16),
    _c("lstm-E-32", "lstm", "E", (2, 1, 8, 8, 0), tile_rows=32),
    _c("lstm-E-split", "lstm", "E", (1, 1, 8, 8, 1), split=True, tile_rows=16),
    _c("lstm-E-split-32", "lstm", "E", (2, 1, 8, 8, 1), split=True, tile_rows=32),
]
BY_ID = {c.id: c for c in CASES}

# (kernel, template arguments) every masked family and branch must be launched at, written out literally
REQUIRED = [
    ("gru_kernel", 1, 1, 2, 1, 4), ("gru_kernel", 2, 1, 2, 1, 4), ("gru_kernel", 1, 2, 4, 0, 8),
    ("gru_kernel", 1, 2, 4, 0, 4), ("gru_kernel", 2, 2, 4, 0, 8), ("gru_kernel", 1, 1, 2, 0, 4),
    ("gru_kernel", 2, 1, 8, 1, 8),
    ("gru2_pipe_kernel", 1, 1, 2, 0, 4), ("gru2_pipe_kernel", 1, 1, 8, 1, 16), ("gru2_pipe_kernel", 2, 1, 8, 1, 16),
    ("gru2_pipe_kernel", 1, 1, 8, 0, 16),
    ("gru_x3_kernel", 1, 1, 2, 1, 4), ("gru_x3_kernel", 2, 1, 2, 1, 4), ("gru_x3_kernel", 1, 1, 2, 0, 4),
    ("gru_x3_kernel", 1, 2, 4, 0, 8), ("gru_x3_kernel", 1, 1, 8, 1, 16), ("gru_x3_kernel", 2, 1, 8, 1, 16),
    ("lstm_kernel", 1, 1, 2, 4, 0), ("lstm_kernel", 2, 1, 2, 4, 0), ("lstm_kernel", 1, 1, 2, 4, 1),
    ("lstm_kernel", 1, 2, 2, 4, 0), ("lstm_kernel", 1, 1, 8, 8, 0), ("lstm_kernel", 2, 1, 8, 8, 0),
    ("lstm_kernel", 1, 1, 8, 8, 1), ("lstm_kernel", 2, 1, 8, 8, 1),
]

# one bidirectional layer of each cell through GruModel / LstmModel: (kind, H, I, seed)
BI = {"gru": ("gru", 64, 24, 231), "lstm": ("lstm", 64, 40, 232)}

# X seeds: the table models' own seed + this; X_SEED would hold a case whose seed had to be changed
# for test_seqlen.py's discrimination condition (none had to)
X_SEED_BASE = 2000
X_SEED = {}


def table(kind):
    return G if kind == "gru" else L


def model(c):
    return table(c.kind).MODELS[c.model]


def weights(c):
    return table(c.kind).weights(c.model)


def dispatch(c):
    """The instance the case's launch resolves to, through the dispatch mirrors of the edge suites
    (a masked launch never takes a cluster path: ws is 0 whatever the pack allows)."""
    m = model(c)
    if c.kind == "gru":
        return G.dispatch(m, rows=ROWS, tile_rows=c.opts.get("tile_rows", 0), pipeline=c.opts.get("pipeline", 1),
                          waves=c.opts.get("waves", 0), ws=0, split=c.split)
    return L.dispatch(m, c.opts.get("tile_rows", 0), c.split)


def instance(c):
    """The case's instance as a REQUIRED entry."""
    return c.inst if c.kind == "gru" else ("lstm_kernel",) + tuple(c.inst)


def lens_for(n, Tn, offset):
    """int32 [n]: the cycle [0, 1, 2, T-1, T, 3, T, 1] from ``offset``, clipped to T."""
    cyc = [0, 1, 2, Tn - 1, Tn, 3, Tn, 1]
    return np.array([min(max(cyc[(offset + i) % 8], 0), Tn) for i in range(n)], np.int32)


def case_lens(c):
    """The case's lengths for all XROWS rows (the per-case offset is its position in CASES)."""
    return lens_for(XROWS, c.T, CASES.index(c))


@lru_cache(maxsize=None)
def case_x(cid):
    """X [T, XROWS, I] float32 of a case (read-only)."""
    c = BY_ID[cid]
    m = model(c)
    seed = X_SEED.get(cid, m.seed + X_SEED_BASE)
    X = np.random.default_rng(seed).standard_normal((c.T, XROWS, m.I)).astype(np.float32)
    X.setflags(write=False)
    return X


def left_align(Xr, lens):
    """Right-aligned zero-padded histories Xr [T, rows, I] (oldest first, the ring gather) with
    ``lens`` live steps per row -> the same histories left-aligned (zeros after the live steps)."""
    Tn = Xr.shape[0]
    X = np.zeros_like(Xr)
    for b, n in enumerate(lens):
        X[:n, b] = Xr[Tn - n:, b]
    return X


def right_align(X, lens):
    """X [T, rows, I] truncated to ``lens`` steps per row and right-aligned: zeros, then the live steps."""
    Tn = X.shape[0]
    Xr = np.zeros_like(X)
    for b, n in enumerate(lens):
        Xr[Tn - n:, b] = X[:n, b]
    return Xr


def masked_ref(kind, layers, head, X, lens, reverse, bf16, dtype=np.float64):
    """(yh [rows, H], out [rows] | None): each row is the kind's unmasked reference (gru_ref / lstm_ref)
    at T = lens[row] on X[:lens[row], row]; a length of 0 leaves the zero state, through the head."""
    ref = G.gru_ref if kind == "gru" else L.lstm_ref
    rows = X.shape[1]
    H = layers[0][1].shape[1]
    yh = np.zeros((rows, H), dtype)
    out = None if head is None else np.zeros(rows, dtype)
    for b in range(rows):
        n = int(lens[b])
        if n > 0:
            y, o = ref(layers, head, X[:n, b:b + 1], reverse=reverse, bf16=bf16, dtype=dtype)
            yh[b] = y[0]
            if head is not None:
                out[b] = o[0]
        elif head is not None:
            w, bias, act = head
            v = dtype(bias)
            out[b] = 1.0 / (1.0 + np.exp(-v)) if act == "sigmoid" else v
    return yh, out


def unmasked_ref(kind, layers, head, X, reverse, bf16, dtype=np.float64):
    ref = G.gru_ref if kind == "gru" else L.lstm_ref
    return ref(layers, head, X, reverse=reverse, bf16=bf16, dtype=dtype)


@lru_cache(maxsize=None)
def reference(cid, dtype_name="float64"):
    """(yh, out) of a case over all XROWS rows, computed once: the bf16-emulating reference for a
    bf16 case, the unrounded one for an f32-faithful (split) case."""
    c = BY_ID[cid]
    layers, head = weights(c)
    return masked_ref(c.kind, layers, head, case_x(cid), case_lens(c), c.reverse, not c.split,
                      dtype=getattr(np, dtype_name))


def tol(c):
    """(yh, out) bounds of a case: the shared constants of the edge suites as they stand."""
    if c.split:
        t = table(c.kind).SPLIT_TOL
        return t, t
    return (G.YH_TOL, G.OUT_TOL) if c.kind == "gru" else L.tol(c.model)


def steps(c):
    """The case's model as masked plan steps: ([GRUStep | LSTMStep, ...], DenseStep head)."""
    from igaming_platform_amd.models.plan import DenseStep, GRUStep, LSTMStep
    m = model(c)
    layers, (wh, bh, act) = weights(c)
    if c.kind == "gru":
        ls = [GRUStep(m.H, W.shape[1], lbr, W, R, B, seq=c.T, masked=True) for W, R, B, lbr in layers]
    else:
        ls = [LSTMStep(m.H, W.shape[1], W, R, B, seq=c.T, masked=True) for W, R, B in layers]
    return ls, DenseStep(1, m.H, act, wh[None, :], np.array([bh], np.float32))


@lru_cache(maxsize=None)
def bi_weights(kind):
    """(forward layer, reverse layer) of the bidirectional model of ``kind`` (no head: Y_h is compared)."""
    _, H, I, seed = BI[kind]
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(H)
    g = 3 if kind == "gru" else 4

    def layer():
        w = (rng.uniform(-s, s, (g * H, I)).astype(np.float32), rng.uniform(-s, s, (g * H, H)).astype(np.float32),
             rng.uniform(-s, s, 2 * g * H).astype(np.float32))
        return w + (1,) if kind == "gru" else w
    return layer(), layer()


@lru_cache(maxsize=None)
def bi_x(kind):
    _, H, I, seed = BI[kind]
    X = np.random.default_rng(seed + X_SEED_BASE).standard_normal((T, XROWS, I)).astype(np.float32)
    X.setflags(write=False)
    return X


def bi_ref(kind, lens, bf16=False):
    """float64 Y_h [rows, 2H] (the ONNX [N, 2, H] order) of the bidirectional model under ``lens``."""
    fwd, rev = bi_weights(kind)
    yf, _ = masked_ref(kind, [fwd], None, bi_x(kind), lens, False, bf16)
    yr, _ = masked_ref(kind, [rev], None, bi_x(kind), lens, True, bf16)
    return np.concatenate([yf, yr], 1)


def bi_onnx(kind, layout=0):
    """Serialized bidirectional model with the sequence_lens input, no head (output: Y_h as [N, 2H])."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model as mk, node, tensor, value_info
    _, H, I, _ = BI[kind]
    fwd, rev = bi_weights(kind)
    attrs = dict(hidden_size=H, direction="bidirectional")
    if kind == "gru":
        attrs["linear_before_reset"] = 1
    if layout:
        attrs["layout"] = 1
    nodes = [node(kind.upper(), ["input", "W", "R", "B", "sequence_lens"], ["Y", "Yh"], **attrs)]
    last = "Yh"
    if not layout:
        nodes.append(node("Transpose", ["Yh"], ["hT"], perm=[1, 0, 2]))
        last = "hT"
    nodes.append(node("Reshape", [last, "shp"], ["output"]))
    inits = [tensor(k, np.stack([a, b])) for k, a, b in zip("WRB", fwd[:3], rev[:3])]
    inits.append(tensor("shp", np.array([-1, 2 * H], np.int64)))
    x_dims = ["N", T, I] if layout else [T, "N", I]
    return mk(nodes, [value_info("input", S.FLOAT, x_dims), value_info("sequence_lens", S.INT32, ["N"])],
              [value_info("output", S.FLOAT, ["N", 2 * H])], inits, name=f"seqlen_bi_{kind}",
              metadata={"family": kind}).SerializeToString()
