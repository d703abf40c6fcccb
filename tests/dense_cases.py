"""Cases, operands and float64 references for the K3 edge tests (tests/test_dense_edges.py on the
CPU executor, tests/test_dense_edges_gpu.py on the device): the dense / GEMV, join, fused head and
MLP-chain kernels at odd widths, strides wider than the live width and every dispatch path.

Inputs follow tests/test_kernels_gpu.py: X ~ N(0, 1), W ~ N(0, 1 / K), b ~ 0.1 N(0, 1), fixed
seeds, so pre-activations stay O(1). The references are plain float64 numpy; the ``bf16``
convention rounds X and W to bf16 first and every chain layer's activations to bf16 before the
next layer (what the bf16 kernels hold in LDS), with f32-or-better accumulation."""
import numpy as np

SENTINEL = -7.0


# ------------------------------------------------------------------------------ references
def bf16r(a):
    """``a`` rounded to bfloat16 (round to nearest even, torch's conversion), as float64."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32)
    return t.numpy().astype(np.float64)


def act64(name, z):
    z = np.asarray(z, np.float64)
    if name == "relu":
        return np.where(z > 0, z, 0.0)
    if name == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if name == "tanh":
        return np.tanh(z)
    assert name == "none", name
    return z


def _lin(h, W, b, bf16):
    W = bf16r(W) if bf16 else np.asarray(W, np.float64)
    z = h @ W.T
    return z if b is None else z + np.asarray(b, np.float64)


def ref64(X, layers=(), head=None, bf16=False):
    """float64 result of ``layers`` = [(W [N, K], b [N] | None, act), ...] applied to X in order,
    then (optionally) ``head`` = (W1 [N1, K], b1, act1, w2 [N1], b2, act2) -> one column.
    ``bf16``: the bf16 kernels' convention - X and every W rounded to bf16, a layer's activations
    rounded to bf16 when another layer reads them; the head's hidden layer and w2 stay f32."""
    h = bf16r(X) if bf16 else np.asarray(X, np.float64)
    for i, (W, b, act) in enumerate(layers):
        h = act64(act, _lin(h, W, b, bf16))
        if bf16 and (i + 1 < len(layers) or head is not None):
            h = bf16r(h)
    if head is not None:
        W1, b1, act1, w2, b2, act2 = head
        h = act64(act1, _lin(h, W1, b1, bf16))
        h = act64(act2, h @ np.asarray(w2, np.float64) + float(b2))[:, None]
    return h


def ref_join(op, A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return A + B if op == "add" else np.concatenate([A, B], 1)


# ------------------------------------------------------------------------------ operands
def poisoned(M_alloc, M, ld, width, dtype, data):
    """[M_alloc, ld] tensor of ``dtype`` whose live block [:M, :width] is ``data`` and whose every
    other element (columns width..ld, rows M..M_alloc) is NaN: a kernel that reads past K or past
    the live rows turns its output NaN."""
    import torch
    t = torch.full((M_alloc, ld), float("nan"), dtype=dtype)
    t[:M, :width] = torch.from_numpy(np.ascontiguousarray(data, np.float32)[:M, :width]).to(dtype)
    return t


def sentinel_out(M_alloc, ld, dtype):
    import torch
    return torch.full((M_alloc, ld), SENTINEL, dtype=dtype)


def untouched(Y, M, N):
    """True when every element of ``Y`` outside [:M, :N] still is the sentinel, bit for bit."""
    import torch
    mask = torch.ones(Y.shape, dtype=torch.bool)
    mask[:M, :N] = False
    ref = torch.full((), SENTINEL, dtype=Y.dtype)
    bits = {2: torch.int16, 4: torch.int32}[Y.element_size()]
    return bool(torch.all(Y.cpu().view(bits)[mask] == ref.view(bits)))


# ------------------------------------------------------------------------------ case tables
# (M, N, K, act, xbf): what each row reaches is the comment; both tile sizes of gemm_kernel, the
# f32 kernel and the GEMV take the same rows (the weight dtype is the test's precision parameter)
DENSE_CASES = [
    (1, 33, 30, "relu", False),       # K % 8 tail, N tail, the sklearn width
    (65, 100, 100, "tanh", False),    # 2 k-tiles (bf16) / 4 (f32) with the last partial, K % 8 = 4, M tail of 1
    (63, 130, 72, "sigmoid", True),   # bf16 A tail path (x_bf16 loaders), N tail of 2 in the third column tile
    (70, 64, 7, "none", False),       # K < 8
    (4097, 130, 100, "relu", False),  # gemm_kernel<128,128>: row tail 1, column tail 2, K tail
    (4097, 130, 100, "relu", True),   # ... with the bf16 A loader
    (4097, 128, 64, "none", False),   # gemm_kernel<128,128>: exact N and K
    (37, 1, 100, "sigmoid", False),   # gemv_kernel: K % 64 != 0, ldx > K
    (37, 1, 100, "sigmoid", True),    # ... bf16 X
    (5, 1, 7, "none", False),         # gemv_kernel: K < 64
]
DENSE_YBF16 = (65, 100, 100, "relu", True)   # y_bf16 stores, ldy = 100 and 103


def dense_id(c):
    return "M{}-N{}-K{}-{}{}".format(*c[:4], "-xbf" if c[4] else "")


def dense_operands(case):
    M, N, K = case[:3]
    rng = np.random.default_rng(1000 + M + 7 * N + 131 * K + int(case[4]))
    X = rng.standard_normal((M, K)).astype(np.float32)
    if case[4]:
        X = bf16r(X).astype(np.float32)   # the producer hands bf16 activations: exact in both
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    return X, W, b


# (precision, K, N1, act1, act2, xbf, kernel, w_lds): the kernel launch_mlp_head must pick
HEAD_CASES = [
    ("fp32", 30, 100, "relu", "sigmoid", False, "fast32", 1),   # KP = 32, N1 tail: the sklearn default shape
    ("fp32", 64, 320, "tanh", "none", False, "fast64", 1),      # 5120 W1 chunks (> 2048), n >= 256 loop
    ("fp32", 33, 300, "sigmoid", "sigmoid", False, "fast64", 1),  # KP = 64 with a K tail, N1 tail past 256
    ("fp32", 96, 128, "relu", "none", False, "generic", 1),     # generic f32, W1 in LDS, k_pad = 96
    ("fp32", 100, 64, "tanh", "sigmoid", False, "generic", 1),  # generic f32, W1 in LDS, k_pad = 128, K tail
    ("fp32", 100, 300, "relu", "none", False, "generic", 0),    # generic f32, W1 from global, N1 tail
    ("bf16", 30, 100, "relu", "sigmoid", False, "bf16", 1),     # bf16 head, W1 in LDS, tails
    ("bf16", 100, 500, "tanh", "none", False, "bf16", 0),       # bf16 head, W1 512 x 136 x 2 B > 64 KB
    ("bf16", 72, 130, "relu", "sigmoid", True, "bf16", 1),      # bf16 X element loader
]
HEAD_M = 70


def head_id(c):
    return "{}-K{}-N{}-{}-{}{}".format(*c[:5], "-xbf" if c[5] else "")


def head_operands(K, N1, M=HEAD_M, xbf=False):
    rng = np.random.default_rng(2000 + 3 * K + 17 * N1)
    X = rng.standard_normal((M, K)).astype(np.float32)
    if xbf:
        X = bf16r(X).astype(np.float32)
    W1 = (rng.standard_normal((N1, K)) / np.sqrt(K)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(N1)).astype(np.float32)
    w2 = (rng.standard_normal(N1) / np.sqrt(N1)).astype(np.float32)
    return X, W1, b1, w2, 0.3


def head_dispatch(precision, k_pad, N1):
    """(kernel, w_lds) by the formulas of launch_mlp_head (csrc/kernels/gemm.hip)."""
    n1p = -(-N1 // 64) * 64
    if precision == "fp32":
        w_lds = int(n1p * (k_pad + 4) * 4 <= 96 * 1024)
        if w_lds and k_pad in (32, 64):
            return f"fast{k_pad}", w_lds
        return "generic", w_lds
    return "bf16", int(n1p * (k_pad + 8) * 2 <= 64 * 1024)


# (widths in -> ... -> n1, hidden acts, act2, waves): the MLP chain rows
CHAIN_CASES = {
    "30-64-64": ((30, 64, 64), ("tanh", "relu"), "sigmoid", 4),
    "1-192-64": ((1, 192, 64), ("sigmoid", "tanh"), "none", 4),
    "65-128-256": ((65, 128, 256), ("relu", "sigmoid"), "none", 8),
    "512-512-128": ((512, 512, 128), ("tanh", "tanh"), "sigmoid", 8),
}
CHAIN_N, CHAIN_LIVE = 70, 66


def chain_operands(name, acts=None, act2=None):
    """X [CHAIN_N, in], dense layers [(W, b, act)], head tuple of one chain row."""
    widths, hacts, a2, _ = CHAIN_CASES[name]
    hacts, a2 = acts or hacts, act2 or a2
    rng = np.random.default_rng(3000 + sum(widths))
    X = rng.standard_normal((CHAIN_N, widths[0])).astype(np.float32)
    lay = []
    for k, n, act in zip(widths[:-1], widths[1:], hacts):
        lay.append(((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32),
                    (0.1 * rng.standard_normal(n)).astype(np.float32), act))
    n1 = widths[-1]
    w2 = (rng.standard_normal(n1) / np.sqrt(n1)).astype(np.float32)
    W1, b1, act1 = lay.pop()
    return X, lay, (W1, b1, act1, w2, 0.1, a2)


def chain_steps(lay, head):
    from igaming_platform_amd.models.plan import DenseStep, HeadStep
    steps = [DenseStep(n=W.shape[0], k=W.shape[1], act=act, w_np=W, b_np=b) for W, b, act in lay]
    W1, b1, act1, w2, b2, act2 = head
    steps.append(HeadStep(n1=W1.shape[0], k=W1.shape[1], act1=act1, act2=act2, w1_np=W1, b1_np=b1, w2_np=w2, b2=b2))
    return steps


def saturating_rows(X, W, b, rows, scale=1e4, seed=0, margin=50.0):
    """X with ``rows`` redrawn at ``scale`` x N(0, 1) so the first layer's pre-activations there
    reach about +-scale. A row is redrawn (fixed seed) until every pre-activation is at least
    ``margin`` from 0 in float64: inside |z| < ~20 a sigmoid / tanh is not saturated, and the f32
    rounding of 1e4-sized products (~1e-3 absolute in z) would be a gap of the reference against
    itself, not of the kernel. ``bf16``-exact values, so both conventions see the same X."""
    rng = np.random.default_rng(seed)
    X = np.array(X, np.float32)
    W64, b64 = np.asarray(W, np.float64), np.asarray(b, np.float64)
    Wb = bf16r(W)
    for r in rows:
        for _ in range(1000):
            x = bf16r(scale * rng.standard_normal(X.shape[1]))
            if min(np.abs(W64 @ x + b64).min(), np.abs(Wb @ x + b64).min()) >= margin:
                break
        else:
            raise AssertionError("no saturating row found")
        X[r] = x
    return X


# ------------------------------------------------------------------------------ ONNX twins
def onnx_mlp(layers):
    """Serialized ONNX model input [N, K] -> (Gemm [+ Relu / Sigmoid / Tanh]) per layer -> output;
    ``layers`` = [(W [N, K], b | None, act), ...]."""
    from igaming_platform_amd.onnx import schema as S
    from igaming_platform_amd.onnx.writer import model, node, tensor, value_info
    nodes, inits, cur = [], [], "input"
    for i, (W, b, act) in enumerate(layers):
        last = i == len(layers) - 1
        W = np.asarray(W, np.float32)
        bias = np.zeros(W.shape[0], np.float32) if b is None else np.asarray(b, np.float32)
        inits += [tensor(f"W{i}", np.ascontiguousarray(W.T)), tensor(f"B{i}", bias)]
        z = f"z{i}" if act != "none" or not last else "output"
        nodes.append(node("Gemm", [cur, f"W{i}", f"B{i}"], [z]))
        cur = z
        if act != "none":
            cur = "output" if last else f"a{i}"
            nodes.append(node(act.capitalize(), [z], [cur]))
    k, n = layers[0][0].shape[1], layers[-1][0].shape[0]
    m = model(nodes, [value_info("input", S.FLOAT, ["N", k])], [value_info("output", S.FLOAT, ["N", n])], inits,
              name="dense_edges", metadata={"family": "mlp"})
    return m.SerializeToString()


def head_layers(head):
    """The head tuple as two ONNX / ref64 layers."""
    W1, b1, act1, w2, b2, act2 = head
    return [(W1, b1, act1), (np.asarray(w2, np.float32)[None, :], np.array([b2], np.float32), act2)]


def plan_layers(plan):
    """(layers, head) of a compiled dense / head plan, for :func:`ref64`."""
    lay, head = [], None
    for s in plan.steps:
        if s.kind == "dense":
            lay.append((s.w_np, s.b_np, s.act))
        else:
            assert s.kind == "head", s.kind
            head = (s.w1_np, s.b1_np, s.act1, s.w2_np, s.b2, s.act2)
    return lay, head


MODEL_CASES = [
    ("mlp_classifier", dict(n_features=30, hidden=100), ["head"]),
    # 100 % 64 != 0: no fused chain; dense then head, the head reading rows of ldx = 100
    ("ltv_mlp", dict(n_features=30, width=100, layers=2), ["dense", "head"]),
    # ... and a dense layer reading them: bf16 rows 200 bytes apart (gemm_kernel's x_bf16 loader)
    ("ltv_mlp", dict(n_features=30, width=100, layers=3), ["dense", "dense", "head"]),
]
