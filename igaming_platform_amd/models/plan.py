"""ONNX graph -> device execution plan.

The C++ reader parses the file; this module lowers the nodes the primary output depends on
(one model input; chains and DAGs whose branches meet in an Add / Concat) to fused device
steps:

* ``TreeStep``   TreeEnsemble{Classifier,Regressor}, or the opset-5 TreeEnsemble with its
                 set-membership splits (``sets``: the member-set table, checked on the host
                 before upload), (+ a following Sigmoid folded into the post transform) -> K2
                 ``tree_ensemble`` on the complete-tree layout, or K2b
                 ``tree_sparse`` on the pointer layout for deep (> 12) or very unbalanced trees,
                 MIN / MAX aggregates and target counts the complete kernel is not built for.
                 Every post transform (NONE, LOGISTIC, SOFTMAX, SOFTMAX_ZERO, PROBIT) runs on
                 the device.
* ``DenseStep``  Gemm / MatMul(+Add) with a following Relu/Sigmoid/Tanh fused into the
                 epilogue -> K3 ``gemm`` (MFMA) or ``gemv`` (N == 1).
* ``GRUStep``    ONNX GRU (forward / reverse / bidirectional, layout 0 / 1) -> K4 (cfg 5). A
                 ``sequence_lens`` input that is an int32 graph input [N] (``Plan.lens_input``, the
                 same for every layer; LSTM alike) lowers to masked steps: K4's masked kernels.
* ``LSTMStep``   ONNX LSTM (same directions / layouts, default activations, no peepholes) -> K4
                 ``lstm`` (csrc/kernels/lstm.hip).
* ``JoinStep``   Add / Concat of two branches (residual blocks, wide & deep) -> ``join``.
* ``RowStep``    LayerNormalization (last axis), Softmax (feature axis), the activations the
                 dense epilogue does not carry (LeakyRelu, Elu, Selu, Softplus, HardSigmoid, Gelu,
                 PRelu, Clip) and a Relu / Sigmoid / Tanh with no dense layer to fold into (after
                 a join, a tree, another activation) -> ``row_op`` (csrc/kernels/rowops.hip).
                 A Softmax over the two logits of an exclusive dense layer is narrowed to
                 sigmoid(z1 - z0) instead, so a two-logit classifier runs on the fused head.
* QDQ int8-quantised models (the standard ai.onnx format of ORT's static quantiser and of QAT
  exports; opset 10 and 13 forms) lower to three step kinds, none of which depends on ``precision``:
  ``QDenseStep``   DequantizeLinear(a) -> Gemm / MatMul on a DequantizeLinear-ed int8 / uint8
                   initializer (per tensor, or per output channel on either axis, so ``transB``
                   works), bias as a DequantizeLinear-ed int32 initializer, a float initializer or
                   MatMul + Add, ``alpha`` / ``beta`` folded, a Relu / Sigmoid / Tanh and a
                   following QuantizeLinear (when it is the only reader) in the epilogue -> K3
                   ``qgemm`` on the i8 matrix cores (csrc/kernels/qgemm.hip); :func:`qdense_tables`
                   builds its host tables. The output is the requantised bytes, else f32 (bf16
                   under the runner's rule for bf16 plans).
  ``QuantStep`` / ``DequantStep``  the two ops on their own (``quantize_rows`` /
                   ``dequantize_rows``): a Q at the model input, after a tree, a join, a row op or
                   on a value with other readers; a DQ that feeds anything but a quantised Gemm. So
                   any float sub-graph lowered here may sit between a DQ and a Q.
  Limits: scales and zero points are initializers; activations are quantised per tensor;
  ``w_q - z_w`` must fit int8; K <= 32768 (the int32 accumulator bound). The QOperator format
  (QLinearMatMul ...), MatMulInteger / DynamicQuantizeLinear, ``block_size``, 4-bit / 16-bit /
  float8 types and ``saturate=0`` raise :class:`PlanError`.
* ``SVMStep``    ai.onnx.ml SVMRegressor (SVR, one-class) and the two-class SVC form of
                 SVMClassifier, kernels LINEAR / POLY / RBF / SIGMOID -> ``svm`` on the f32 matrix
                 cores (csrc/kernels/svm.hip), f32 whatever ``precision`` says. A Scaler / constant
                 affine on its input folds into the step's input stage, a following constant Mul /
                 Add / Neg and a Sigmoid into its epilogue (exclusive, single-use values only, as the
                 tree Sigmoid fold); a classifier is lowered to its positive column. Up to
                 ``SVM_MAX_F`` = 256 input columns; POLY with an integral degree in [0, 16]; post
                 transforms NONE and LOGISTIC; anything else raises :class:`PlanError`.
* ``ColumnStep`` the front end of a scikit-learn ``Pipeline(ColumnTransformer, estimator)``: any
                 sub-graph of ai.onnx.ml Imputer, Scaler, OneHotEncoder, Binarizer,
                 ArrayFeatureExtractor, FeatureVectorizer and ai.onnx Gather / Slice (feature axis,
                 constant indices), Concat (axis 1) and Cast(int) -> OneHotEncoder is tracked as a
                 *column view* - per column of the value, a record (source column of a base value,
                 impute, (x - sub) * mul, pass | one-hot | binarize) - and becomes ONE
                 ``col_assemble`` launch (csrc/kernels/columns.hip) when anything else reads it. An
                 operator that does not fit the record's free stages materialises the view and
                 starts a fresh one, so float arithmetic is never reordered and the step is
                 bit-equal to the executor. Up to 256 base columns and 4096 assembled ones; string
                 categories, ``zeros = 0`` and the int64 Imputer attributes raise :class:`PlanError`.
* ``ConvStep`` / ``SeqPoolStep``  temporal-convolution (Conv1D / TCN) sequence models: the 3-D model input goes
                 through ``Transpose`` (perm [1, 2, 0] for layout 0, [0, 2, 1] for layout 1) into a *sequence
                 value*, logically [N, C, T]. Each ONNX ``Conv`` (1-D, stride 1, group 1, constant W) on one
                 becomes a ``ConvStep`` of output length T -> ``conv1d`` (csrc/kernels/conv1d.hip, f32 whatever
                 ``precision`` says); ``pads``, ``auto_pad``, a constant-zero ``Pad`` in front and a ``Slice`` (step
                 1) behind compose into its ``pad_left``. A following Relu / Sigmoid / Tanh, a residual ``Add``
                 with another sequence value (then the activation behind it) and an inference
                 BatchNormalization fold into the step, under the exclusivity rule of the dense folds; Dropout /
                 Identity fold away. GlobalAveragePool / GlobalMaxPool, Reduce{Mean,Max,Sum} over axis 2,
                 Gather(axis 2, last index) and Slice[T - 1 : T] give the ``SeqPoolStep`` read-out (``seq_pool``),
                 after which the value is an ordinary [N, C] one: dense layers follow. Limits ``CONV_MAX_C`` = 256
                 channels, ``CONV_MAX_K`` = 8 taps, ``CONV_MAX_SPAN`` = 128 = dil (k - 1), ``CONV_MAX_T`` = 1024
                 steps. Any other operator on a sequence value, a length other than T, a non-zero pad value,
                 padding on N or C, a strided cut, GRU / LSTM layers in the same model raise :class:`PlanError`.
* ``BatchNormalization`` (inference) is a per-column affine and folds like ``Scaler``;
  ``Dropout`` is folded away.
* ai.onnx.ml ``LinearClassifier`` / ``LinearRegressor`` (post NONE / LOGISTIC; a two-class
  SOFTMAX as sigmoid(s1 - s0)) -> a dense layer, so an sklearn pipeline
  Scaler -> LinearClassifier -> ZipMap, or an MLP ending in one, runs on the fused head.
* ``Scaler`` and constant Add / Sub / Mul / Div fold into a neighbouring dense layer's
  weights; Identity / Flatten / Squeeze / Reshape / ZipMap / Cast(float) are folded away.

Anything else raises :class:`PlanError`; the engine then runs that model through the C++
CPU executor (explicitly, with a warning) rather than silently substituting torch ops.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ..native import native

ML_DOMAIN = "ai.onnx.ml"
POST = {0: "NONE", 1: "LOGISTIC", 2: "SOFTMAX", 3: "SOFTMAX_ZERO", 4: "PROBIT"}
ONNX_INT32 = 6   # TensorProto.DataType of a graph input's element type


class PlanError(RuntimeError):
    pass


@dataclass
class TreeStep:
    n_trees: int
    depth: int
    k: int
    n_out: int
    post: int            # kernel post code (POST): 0 none, 1 logistic, 2 softmax, 3 softmax_zero, 4 probit
    average: int
    binary_class: int    # -1 unless the classifier binary case
    all_positive: int
    max_feature: int
    nodes_np: np.ndarray  # complete: [T][2^D-1][2] f32; sparse: [N][4] int32
    leaves_np: Optional[np.ndarray]  # complete: [T][2^D][K]; sparse: None
    base_np: Optional[np.ndarray]
    classifier: bool = False
    layout: str = "complete"   # complete (K2) | sparse (K2b pointer layout)
    aggregate: int = 0         # 0 sum, 1 average, 2 min, 3 max
    roots_np: Optional[np.ndarray] = None     # sparse: [T] root node index
    leaf_w_np: Optional[np.ndarray] = None    # sparse: [L][K]
    leaf_has_np: Optional[np.ndarray] = None  # sparse: [L][K] uint8
    sets_np: Optional[np.ndarray] = None      # uint32 member-set table of the BRANCH_MEMBER nodes
    sets: Any = None                          # device copy (int32 view); None when the table is empty
    nodes: Any = None
    leaves: Any = None
    base: Any = None
    roots: Any = None
    leaf_w: Any = None
    leaf_has: Any = None
    kind: str = "tree"
    src: Optional[int] = None  # producing step of the input (None: the previous step; -1: model input)

    @property
    def out_width(self) -> int:
        return self.n_out

    @property
    def all_leq(self) -> bool:
        """Every node is BRANCH_LEQ (sklearn-style ensembles; missing-value tracks allowed): the
        kernel then skips decoding the comparison mode per node."""
        if self.layout != "complete":
            return False
        meta = self.nodes_np.reshape(-1, 2)[:, 1].view(np.uint32)
        return bool(np.all(((meta >> 16) & 0x7) == 0))


COMPLETE_K = (1, 2, 4, 8, 16, 32, 64)   # target counts the complete-tree kernel is built for
SPARSE_MAX_K = 64


def choose_tree_layout(info: Dict[str, Any], depth_limit: int = 12) -> str:
    """complete (K2) when the ensemble fits it without much padding, else sparse (K2b).
    ``IGP_TREE_LAYOUT=complete|sparse`` forces one (the complete layout still needs SUM /
    AVERAGE, depth <= ``depth_limit`` and a supported K)."""
    import os
    D, T, N, K = int(info["depth"]), int(info["n_trees"]), int(info["n_nodes"]), int(info["k"])
    fits = int(info["aggregate"]) in (0, 1) and D <= depth_limit and K in COMPLETE_K
    forced = os.environ.get("IGP_TREE_LAYOUT", "auto")
    if forced == "sparse" or not fits:
        return "sparse"
    if forced == "complete":
        return "complete"
    # the complete layout stores 2^(D+1) - 1 slots per tree: keep it when that is within 8x
    # of the real node count (balanced GBDTs are ~1x; a few deep paths blow it up)
    return "complete" if T * ((1 << (D + 1)) - 1) <= 8 * max(N, 1) + 64 * T else "sparse"


@dataclass
class DenseStep:
    n: int
    k: int
    act: str
    w_np: np.ndarray     # [N, K] float32 (logical)
    b_np: Optional[np.ndarray]
    w: Any = None        # bf16 [N_pad, K_pad] device
    b: Any = None
    kind: str = "dense"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.n


@dataclass
class HeadStep:
    """dense(K -> N1, act1) + dense(N1 -> 1, act2) fused into one kernel (K3 mlp_head)."""
    n1: int
    k: int
    act1: str
    act2: str
    w1_np: np.ndarray    # [N1, K]
    b1_np: Optional[np.ndarray]
    w2_np: np.ndarray    # [N1]
    b2: float
    w1: Any = None
    b1: Any = None
    w2: Any = None
    kind: str = "head"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return 1


@dataclass
class GRUStep:
    hidden: int
    in_dim: int
    linear_before_reset: int
    w_np: np.ndarray     # [3H, I]
    r_np: np.ndarray     # [3H, H]
    b_np: np.ndarray     # [6H]
    seq: int = 0
    dev: Dict[str, Any] = field(default_factory=dict)
    kind: str = "gru"
    src: Optional[int] = None
    reverse: bool = False      # direction=reverse: the sequence is read last step first
    layout: int = 0            # ONNX layout attribute (1: batch-major X / Y / Y_h)
    bidirectional: bool = False
    w_rev_np: Optional[np.ndarray] = None  # bidirectional: the reverse direction's W / R / B
    r_rev_np: Optional[np.ndarray] = None
    b_rev_np: Optional[np.ndarray] = None
    masked: bool = False       # the node reads sequence_lens (Plan.lens_input): short rows hold their state

    @property
    def out_width(self) -> int:
        return self.hidden * (2 if self.bidirectional else 1)

    def direction(self, d: int) -> "GRUStep":
        """One direction of a bidirectional layer as a unidirectional step (d = 1: reverse)."""
        if d == 0:
            return GRUStep(self.hidden, self.in_dim, self.linear_before_reset, self.w_np, self.r_np, self.b_np,
                           seq=self.seq, layout=self.layout, masked=self.masked)
        return GRUStep(self.hidden, self.in_dim, self.linear_before_reset, self.w_rev_np, self.r_rev_np,
                       self.b_rev_np, seq=self.seq, reverse=True, layout=self.layout, masked=self.masked)


@dataclass
class LSTMStep:
    """One ONNX LSTM layer (gate order i, o, f, c; sigmoid / tanh / tanh; zero initial states)."""
    hidden: int
    in_dim: int
    w_np: np.ndarray     # [4H, I]
    r_np: np.ndarray     # [4H, H]
    b_np: np.ndarray     # [8H]: Wb i,o,f,c | Rb i,o,f,c
    seq: int = 0
    kind: str = "lstm"
    src: Optional[int] = None
    reverse: bool = False
    layout: int = 0
    bidirectional: bool = False
    w_rev_np: Optional[np.ndarray] = None
    r_rev_np: Optional[np.ndarray] = None
    b_rev_np: Optional[np.ndarray] = None
    masked: bool = False       # as GRUStep.masked (h and c are held)

    @property
    def out_width(self) -> int:
        return self.hidden * (2 if self.bidirectional else 1)

    def direction(self, d: int) -> "LSTMStep":
        """One direction of a bidirectional layer as a unidirectional step (d = 1: reverse)."""
        if d == 0:
            return LSTMStep(self.hidden, self.in_dim, self.w_np, self.r_np, self.b_np, seq=self.seq,
                            layout=self.layout, masked=self.masked)
        return LSTMStep(self.hidden, self.in_dim, self.w_rev_np, self.r_rev_np, self.b_rev_np, seq=self.seq,
                        reverse=True, layout=self.layout, masked=self.masked)


SEQUENCE_KINDS = ("gru", "lstm", "conv")   # recurrent / convolution steps: the plan is then a sequence model
RECURRENT_KINDS = ("gru", "lstm")


def is_sequence_step(s) -> bool:
    return s.kind in SEQUENCE_KINDS


def has_sequence(steps) -> bool:
    """Whether the steps form a sequence model (GRU / LSTM layers, K4, or the convolution layers of
    a TCN: [T, rows, I] input)."""
    return any(is_sequence_step(s) for s in steps or ())


@dataclass
class Plan:
    family: str
    in_width: int
    steps: List[Any]
    out_width: int
    ml_col: int
    metadata: Dict[str, str]
    input_name: str
    output_name: str
    seq_input: bool = False
    precision: str = "fp32"   # dense / head weights on device: fp32 (reference, f32 MFMA) | bf16
    cpu_col: Optional[int] = None  # score column in the CPU executor's output (None: ml_col)
    # the int32 [N] graph input every GRU / LSTM layer reads as ONNX sequence_lens (None: no masking)
    lens_input: Optional[str] = None

    @property
    def executor_col(self) -> int:
        """Column of the model score in the C++ executor's output tensor (a binary classifier
        lowered to its positive column has ml_col 0 on the device, 1 in the executor)."""
        return self.ml_col if self.cpu_col is None else self.cpu_col

    @property
    def is_chain(self) -> bool:
        return all(s.kind != "join" and getattr(s, "src", None) is None for s in self.steps)

    def describe(self) -> str:
        parts = []
        for s in self.steps:
            if s.kind == "tree":
                parts.append(f"tree(T={s.n_trees},D={s.depth},K={s.k},post={s.post},{s.layout})")
            elif s.kind == "dense":
                parts.append(f"dense({s.k}->{s.n},{s.act})")
            elif s.kind == "head":
                parts.append(f"head({s.k}->{s.n1},{s.act1}->1,{s.act2})")
            elif s.kind == "join":
                parts.append(f"{s.op}(#{s.a},#{s.b})")
            elif s.kind == "row":
                parts.append(f"{s.act if s.op == 'act' else s.op}({s.width})")
            elif s.kind == "qdense":
                parts.append(f"qdense({s.x_type}:{s.k}->{s.n},{s.act},{s.out_q[2] if s.out_q else 'f32'})")
            elif s.kind in ("quant", "dequant"):
                parts.append(f"{s.kind}({s.width},{s.qtype})")
            elif s.kind == "svm":
                parts.append(f"svm({s.in_dim},{s.n_sv},{s.kernel})")
            elif s.kind == "cols":
                parts.append(f"cols({s.in_width}->{s.out_width})")
            elif s.kind == "conv":
                parts.append(f"conv({s.c_in}->{s.c_out},k={s.k},d={s.dil},p={s.pad_left})")
            elif s.kind == "seqpool":
                parts.append(f"seqpool({s.op},{s.width})")
            else:
                parts.append(f"{s.kind}(I={s.in_dim},H={s.hidden}{',lens' if getattr(s, 'masked', False) else ''})")
        return " -> ".join(parts)


@dataclass
class JoinStep:
    """Add / Concat of two branch values (join.hip): ``a`` / ``b`` are the producing steps'
    indices (-1: the model input). Residual blocks and wide & deep towers lower to one per
    join; everything else in the branches stays on the fused dense / tree / head kernels."""
    op: str      # add | concat
    a: int
    b: int
    na: int
    nb: int
    kind: str = "join"

    @property
    def out_width(self) -> int:
        return self.na if self.op == "add" else self.na + self.nb


@dataclass
class RowStep:
    """A row op on one activation tensor (rowops.hip): ``layernorm`` (gamma, optional beta, eps)
    or ``softmax`` over each row, or ``act`` - an elementwise activation the dense / head epilogues
    do not carry (``ROW_ACTS`` of ops/kernels.py; parameters ``p0`` / ``p1``; a per-column PRelu
    slope in ``gamma_np``), or a Relu / Sigmoid / Tanh that has no dense layer to fold into."""
    op: str      # layernorm | softmax | act
    width: int
    act: str = "none"
    p0: float = 0.0
    p1: float = 0.0
    eps: float = 1e-5
    gamma_np: Optional[np.ndarray] = None
    beta_np: Optional[np.ndarray] = None
    gamma: Any = None
    beta: Any = None
    kind: str = "row"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.width


ONNX_UINT8, ONNX_INT8 = 2, 3
QTYPES = {ONNX_UINT8: "uint8", ONNX_INT8: "int8"}   # quantised element types (by the zero point's type)
Q_OFF = {"uint8": 128, "int8": 0}      # the device stores a quantised value q as the signed byte q - off
Q_RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
Q_MAX_K = 32768                        # qgemm: acc + corr stays inside int32 up to this reduction length
QDQ_ONLY = ("quantised models are lowered in the QDQ format (QuantizeLinear / DequantizeLinear around float "
            "Gemm / MatMul)")


@dataclass
class QDenseStep:
    """DequantizeLinear(a) -> Gemm | MatMul on a ``DequantizeLinear``-ed int8 / uint8 weight, with an
    optional Relu / Sigmoid / Tanh and an optional following QuantizeLinear folded in (K3 ``qgemm``,
    csrc/kernels/qgemm.hip): reads the quantised activation bytes, accumulates in int32, writes
    f32 / bf16 or the requantised bytes (``out_q``). None of it depends on ``precision``."""
    n: int
    k: int
    act: str
    wq_np: np.ndarray            # [N, K] int32: w_q - z_w (inside int8)
    w_scale: np.ndarray          # [N] f32 (a per-tensor scale broadcast)
    alpha: float                 # Gemm alpha (into mult)
    x_scale: np.float32
    x_zp: int
    x_type: str                  # uint8 | int8
    w_np: np.ndarray             # [N, K] f32 dequantised (x alpha), for plan_importance
    b_np: Optional[np.ndarray]   # [N] f32 (Gemm C x beta, an Add constant; dequantised when it was int32)
    out_q: Optional[Tuple[np.float32, int, str]] = None   # folded QuantizeLinear: (s_y, z_y, type)
    w8: Any = None               # device tables (qdense_tables)
    corr: Any = None
    mult: Any = None
    b: Any = None
    kind: str = "qdense"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.n


@dataclass
class QuantStep:
    """QuantizeLinear on its own (``quantize_rows``): f32 / bf16 -> stored bytes, per tensor."""
    width: int
    scale: np.float32
    zp: int
    qtype: str
    kind: str = "quant"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.width


@dataclass
class DequantStep:
    """DequantizeLinear on its own (``dequantize_rows``): stored bytes -> f32 / bf16, per tensor."""
    width: int
    scale: np.float32
    zp: int
    qtype: str
    kind: str = "dequant"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.width


SVM_KERNELS = ("LINEAR", "POLY", "RBF", "SIGMOID")   # csrc/runtime/svm.h Kernel codes
SVM_MAX_F = 256          # input columns the device kernel stages (csrc/kernels/launch.h SVM_MAX_F)
SVM_MAX_DEGREE = 16      # POLY degrees run as a fixed multiply sequence up to here


@dataclass
class SVMStep:
    """ai.onnx.ml SVMRegressor / two-class SVMClassifier (csrc/kernels/svm.hip), f32 whatever the
    plan's precision: dec = sum_i coef[i] K(x', sv_i) + rho on x' = x * in_scale + in_shift, then the
    folded output stage, in this order: Platt p = 1 / (1 + exp(a dec + b)) (``platt_flip``: 1 - p,
    the classifier's positive column), the one-class sign, v * post_scale + post_shift, ``act``.
    The device takes up to ``SVM_MAX_F`` = 256 input columns (its X tile lives in LDS)."""
    kernel: str              # LINEAR | POLY | RBF | SIGMOID
    gamma: float
    coef0: float
    degree: int              # POLY only
    n_sv: int
    in_dim: int
    sv_np: np.ndarray        # [S, F] f32
    coef_np: np.ndarray      # [S] f32
    rho: float
    in_scale: Optional[np.ndarray] = None   # [F] float64: a folded Scaler / constant affine
    in_shift: Optional[np.ndarray] = None
    post_scale: float = 1.0
    post_shift: float = 0.0
    act: str = "none"        # none | sigmoid
    platt: Optional[Tuple[float, float]] = None
    platt_flip: bool = False
    one_class: bool = False
    sv: Any = None           # device tables (svm_tables)
    coef: Any = None
    sv_norm: Any = None
    scale: Any = None
    shift: Any = None
    kind: str = "svm"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return 1


def svm_centre(sv: np.ndarray) -> np.ndarray:
    """The point an RBF step's vectors and inputs are moved by: per column the mean of the support
    vectors, snapped to a power-of-two grid no finer than their largest distance from it (the mean
    itself when they all agree). The residual offset stays within the vectors' spread, and ``s - c``
    is exact for vectors with short mantissas (integer features stay integers)."""
    sv64 = np.asarray(sv, np.float64)
    mean = sv64.mean(axis=0)
    dev = np.abs(sv64 - mean).max(axis=0)
    grid = np.exp2(np.ceil(np.log2(np.where(dev > 0, dev, 1.0))))
    return np.where(dev > 0, np.round(mean / grid) * grid, mean)


def svm_tables(s: SVMStep) -> Dict[str, Any]:
    """Host tables of a kernel machine, as torch tensors on the CPU (no GPU needed):

    * ``sv``      f32 [S_pad(64), f_pad(32)], zero padded; ``coef`` f32 [S_pad];
    * ``scale`` / ``shift`` f32 [f_pad]: the input affine (ones / zeros without one);
    * ``sv_norm`` f32 [S_pad] (RBF only): |s_i|^2 of the table's rows, summed in float64, rounded once.

    RBF runs as |x'|^2 + |s|^2 - 2 x'.s. To keep that away from cancellation on unscaled features
    the problem is centred first: the table holds s_i - c and the shift in_shift - c, c =
    :func:`svm_centre` (distances do not change). The other kernels are not centred."""
    import torch
    S, F = s.sv_np.shape
    sv = s.sv_np.astype(np.float64)
    scale = np.ones(F) if s.in_scale is None else np.broadcast_to(np.asarray(s.in_scale, np.float64), (F,))
    shift = np.zeros(F) if s.in_shift is None else np.broadcast_to(np.asarray(s.in_shift, np.float64), (F,))
    if s.kernel == "RBF":
        c = svm_centre(sv)
        sv, shift = sv - c, shift - c
    s_pad, f_pad = -(-S // 64) * 64, -(-F // 32) * 32
    tab = np.zeros((s_pad, f_pad), np.float32)
    tab[:S, :F] = sv
    coef = np.zeros(s_pad, np.float32)
    coef[:S] = s.coef_np
    sc, sh = np.zeros(f_pad, np.float32), np.zeros(f_pad, np.float32)
    sc[:F], sh[:F] = scale, shift
    out = dict(sv=torch.from_numpy(tab), coef=torch.from_numpy(coef), scale=torch.from_numpy(sc),
               shift=torch.from_numpy(sh), sv_norm=None)
    if s.kernel == "RBF":
        out["sv_norm"] = torch.from_numpy((tab.astype(np.float64) ** 2).sum(axis=1).astype(np.float32))
    return out


def validate_svm(s: SVMStep) -> None:
    """Host check of a kernel machine before it reaches the device: a known kernel, table shapes
    that agree, finite values, and sizes inside what svm.hip is built for."""
    if s.kernel not in SVM_KERNELS:
        raise PlanError(f"svm: unknown kernel type {s.kernel!r}")
    if s.sv_np.ndim != 2 or s.sv_np.shape != (s.n_sv, s.in_dim) or s.coef_np.shape != (s.n_sv,) or s.n_sv < 1:
        raise PlanError("svm: support vectors must be [S, F] with one coefficient each")
    if not 1 <= s.in_dim <= SVM_MAX_F:
        raise PlanError(f"svm: {s.in_dim} input columns (the device kernel takes 1 .. {SVM_MAX_F})")
    if s.kernel == "POLY" and (int(s.degree) != s.degree or not 0 <= s.degree <= SVM_MAX_DEGREE):
        raise PlanError(f"svm: POLY degree {s.degree} (an integer in [0, {SVM_MAX_DEGREE}])")
    if s.act not in ("none", "sigmoid"):
        raise PlanError(f"svm: activation {s.act!r}")
    for name, t in (("support vectors", s.sv_np), ("coefficients", s.coef_np), ("in_scale", s.in_scale),
                    ("in_shift", s.in_shift)):
        if t is not None and not np.isfinite(np.asarray(t, np.float64)).all():
            raise PlanError(f"svm: non-finite {name}")
    for name, t in (("in_scale", s.in_scale), ("in_shift", s.in_shift)):
        if t is not None and np.asarray(t).size not in (1, s.in_dim):
            raise PlanError(f"svm: {name} must hold one value per input column")
    scal = [s.gamma, s.coef0, s.rho, s.post_scale, s.post_shift] + list(s.platt or ())
    if not np.isfinite(np.asarray(scal, np.float64)).all():
        raise PlanError("svm: non-finite parameters")


CONV_MAX_C = 256         # input / output channels of a ConvStep (csrc/kernels/launch.h CONV_MAX_C)
CONV_MAX_K = 8           # taps
CONV_MAX_SPAN = 128      # dil * (k - 1): the halo a time tile stages
CONV_MAX_T = 1024        # time steps
POOL_OPS = {"last": 0, "mean": 1, "max": 2, "sum": 3}   # csrc/kernels/launch.h SeqPoolOp


@dataclass
class ConvStep:
    """One 1-D convolution layer of a temporal-convolution (TCN) sequence model on a sequence value,
    logically [N, C, T] (csrc/kernels/conv1d.hip), f32 whatever the plan's precision. The output
    length is always T:

        out[o, t] = b[o] + sum_j sum_c W[o, c, j] * x[c, t - pad_left + j * dil]     (zero outside [0, T))

    then ``act``, then ``+ res`` (the output of step ``res``, a sequence value of c_out channels; None:
    nothing is added; the model input, -1, is not allowed), then ``act_post``."""
    c_in: int
    c_out: int
    k: int
    dil: int
    pad_left: int
    w_np: np.ndarray          # [C_out, k, C_in] f32
    b_np: np.ndarray          # [C_out] f32
    act: str = "none"
    res: Optional[int] = None
    act_post: str = "none"
    seq: int = 0
    layout: int = 0           # of the model input: 0 [T, N, I], 1 [N, T, I]
    w: Any = None             # device tables (conv_tables)
    b: Any = None
    kind: str = "conv"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.c_out


@dataclass
class SeqPoolStep:
    """The read-out of a sequence value [N, C, T] -> [N, C] (``seq_pool`` of conv1d.hip): ``last``
    (step T - 1), ``mean`` / ``sum`` / ``max`` over t ascending; a NaN in the column makes ``max`` NaN."""
    op: str
    width: int
    seq: int = 0
    layout: int = 0
    kind: str = "seqpool"
    src: Optional[int] = None

    @property
    def out_width(self) -> int:
        return self.width


def check_conv(s: ConvStep) -> None:
    """Host check of a convolution layer against what conv1d.hip is built for."""
    if not (1 <= s.c_in <= CONV_MAX_C and 1 <= s.c_out <= CONV_MAX_C):
        raise PlanError(f"conv: {s.c_in} -> {s.c_out} channels (the device kernel takes 1 .. {CONV_MAX_C})")
    if not 1 <= s.k <= CONV_MAX_K:
        raise PlanError(f"conv: kernel size {s.k} (the device kernel takes 1 .. {CONV_MAX_K})")
    if s.dil < 1 or s.dil * (s.k - 1) > CONV_MAX_SPAN:
        raise PlanError(f"conv: dilation {s.dil} x (k - 1) = {s.dil * (s.k - 1)} (the device kernel takes up to {CONV_MAX_SPAN})")
    if not 1 <= s.seq <= CONV_MAX_T:
        raise PlanError(f"conv: {s.seq} time steps (the device kernel takes 1 .. {CONV_MAX_T})")
    if not 0 <= s.pad_left <= s.dil * (s.k - 1):
        raise PlanError(f"conv: left padding {s.pad_left} outside [0, dil (k - 1) = {s.dil * (s.k - 1)}]")
    if s.w_np.shape != (s.c_out, s.k, s.c_in) or s.b_np.shape != (s.c_out,):
        raise PlanError("conv: weights must be [C_out, k, C_in] with one bias per output channel")
    if s.act not in ACT_NAMES or s.act_post not in ACT_NAMES:
        raise PlanError(f"conv: activation {s.act!r} / {s.act_post!r}")
    if s.res is not None and s.res < 0:
        raise PlanError("conv: the residual must be the output of a step (not the model input)")


ACT_NAMES = ("none", "relu", "sigmoid", "tanh")


def conv_tables(s: ConvStep) -> Dict[str, Any]:
    """Host tables of a convolution layer, as torch tensors on the CPU (no GPU needed):

    * ``w``    f32 [ceil(C_out / 16), k, ceil(C_in / 16), 64, 4] in MFMA fragment order: element
      (ob, j, kc, lane, e) is W[ob * 16 + (lane & 15), kc * 16 + 4 * (lane >> 4) + e, j], zero past
      C_out / C_in - one wave load of a fragment is 1 KiB contiguous;
    * ``bias`` f32 [round_up(C_out, 16)], zeros past C_out."""
    import torch
    n_ob, n_kc = -(-s.c_out // 16), -(-s.c_in // 16)
    wp = np.zeros((n_ob * 16, s.k, n_kc * 16), np.float32)
    wp[:s.c_out, :, :s.c_in] = s.w_np
    # [ob, li, j, kc, g, e] -> [ob, j, kc, g, li, e]; lane = 16 g + li
    frag = wp.reshape(n_ob, 16, s.k, n_kc, 4, 4).transpose(0, 2, 3, 4, 1, 5)
    bias = np.zeros(n_ob * 16, np.float32)
    bias[:s.c_out] = s.b_np
    return dict(w=torch.from_numpy(np.ascontiguousarray(frag).reshape(n_ob, s.k, n_kc, 64, 4)), bias=torch.from_numpy(bias))


COL_MODES = {"pass": 0, "onehot": 1, "binarize": 2, "zero": 3}   # csrc/kernels/launch.h ColMode
COL_IMPUTE, COL_IMP_NAN, COL_AFFINE = 0x10, 0x20, 0x40          # ... and the ColRecord flag bits
COL_MAX_IN = 256         # widest base value the kernel stages (csrc/kernels/launch.h COL_MAX_IN)
COL_MAX_OUT = 4096
COL_RECORD = np.dtype([("src", "<i4"), ("flags", "<i4"), ("replaced", "<f4"), ("value", "<f4"), ("sub", "<f4"),
                       ("mul", "<f4"), ("arg", "<f4"), ("pad", "<f4")])   # launch.h ColRecord, 32 bytes


@dataclass(frozen=True)
class ColRec:
    """One column of a column view: a function of column ``src`` of the base value, evaluated in
    this order: impute (``imp`` = (replaced, value): x = hit ? value : x, hit = isnan(x) for a NaN
    ``replaced``, else x == replaced), the affine (``aff`` = (sub, mul): (x - sub) * mul in f32, the
    Scaler's own order), then ``mode``: pass | onehot (trunc(x) == arg) | binarize (x > arg) | zero."""
    src: int
    imp: Optional[Tuple[float, float]] = None
    aff: Optional[Tuple[float, float]] = None
    mode: str = "pass"
    arg: float = 0.0

    @property
    def identity(self) -> bool:
        return self.imp is None and self.aff is None and self.mode == "pass"


@dataclass
class ColumnStep:
    """A sub-graph of column operators (Imputer, Scaler, OneHotEncoder, Binarizer,
    ArrayFeatureExtractor / Gather / Slice, Concat / FeatureVectorizer: a scikit-learn
    ColumnTransformer) as one launch of ``col_assemble`` (csrc/kernels/columns.hip): output column
    j is ``records[j]`` of the producing value's row. f32 in; the arithmetic is the CPU executor's,
    so the result is bit-equal to it."""
    in_width: int
    out_width: int
    records: List[ColRec]
    tab: Any = None          # device table (upload_columns)
    tab_key: Any = None      # what the table was checked and built for: (in_width, out_width, id(records))
    kind: str = "cols"
    src: Optional[int] = None


def column_table(s: ColumnStep) -> np.ndarray:
    """The step's record table as the kernel reads it: one ``COL_RECORD`` per output column, padded
    to a multiple of 4 columns with always-zero records."""
    tab = np.zeros(-(-len(s.records) // 4) * 4, COL_RECORD)
    tab["flags"] = COL_MODES["zero"]
    for j, r in enumerate(s.records):
        flags = COL_MODES[r.mode]
        if r.imp is not None:
            rep, val = np.float32(r.imp[0]), np.float32(r.imp[1])
            flags |= COL_IMPUTE | (COL_IMP_NAN if np.isnan(rep) else 0)
            tab[j]["replaced"], tab[j]["value"] = (0.0 if np.isnan(rep) else rep), val
        if r.aff is not None:
            flags |= COL_AFFINE
            tab[j]["sub"], tab[j]["mul"] = np.float32(r.aff[0]), np.float32(r.aff[1])
        tab[j]["src"], tab[j]["flags"], tab[j]["arg"] = r.src, flags, np.float32(r.arg)
    return tab


def check_columns(s: ColumnStep) -> None:
    """Host check of a column step before it reaches the device: sizes inside what columns.hip is
    built for, every source column inside the base value, known modes, finite constants where the
    kernel compares or multiplies with them (an imputed value may be anything; a replaced value may
    be NaN: that is the isnan test)."""
    if not 1 <= int(s.in_width) <= COL_MAX_IN:
        raise PlanError(f"cols: {s.in_width} input columns (the device kernel takes 1 .. {COL_MAX_IN})")
    if not 1 <= int(s.out_width) <= COL_MAX_OUT or len(s.records) != s.out_width:
        raise PlanError(f"cols: {s.out_width} output columns with {len(s.records)} records (1 .. {COL_MAX_OUT}, one each)")
    for j, r in enumerate(s.records):
        if int(r.src) != r.src or not 0 <= r.src < s.in_width:
            raise PlanError(f"cols: column {j} reads source column {r.src} of {s.in_width}")
        if r.mode not in COL_MODES:
            raise PlanError(f"cols: column {j} has unknown mode {r.mode!r}")
        if r.imp is not None and len(r.imp) != 2:
            raise PlanError(f"cols: column {j} has a malformed impute stage {r.imp!r}")
        if r.aff is not None and (len(r.aff) != 2 or not np.isfinite(np.asarray(r.aff, np.float32)).all()):
            raise PlanError(f"cols: column {j} has a non-finite affine stage {r.aff!r}")
        if r.mode in ("onehot", "binarize") and not np.isfinite(np.float32(r.arg)):
            raise PlanError(f"cols: column {j} compares with a non-finite constant")
        if r.mode == "onehot" and (np.float32(r.arg) != np.trunc(np.float32(r.arg)) or abs(float(r.arg)) >= 2.0 ** 63):
            raise PlanError(f"cols: column {j} has one-hot category {r.arg!r} (an integer inside (-2^63, 2^63))")


def columns_key(s: ColumnStep):
    """What a step's uploaded table stands for; the launch wrapper compares it in O(1), so the
    per-record check runs once, at upload."""
    return (int(s.in_width), int(s.out_width), id(s.records))


def upload_columns(s: ColumnStep, device) -> None:
    """Check the step on the host (:func:`check_columns`), then build and upload its record table."""
    import torch
    check_columns(s)
    s.tab = torch.from_numpy(column_table(s).view(np.uint8).reshape(-1, COL_RECORD.itemsize)).to(device)
    s.tab_key = columns_key(s)


def step_qtype(s) -> Optional[str]:
    """The quantised type of a step's output buffer (None: a float buffer)."""
    if s.kind == "quant":
        return s.qtype
    if s.kind == "qdense" and s.out_q is not None:
        return s.out_q[2]
    return None


def qdense_tables(s: QDenseStep) -> Dict[str, Any]:
    """Host tables of a quantised dense layer, as torch tensors on the CPU (no GPU needed):

    * ``w8``   int8 [N_pad(128), K_pad(64)]: w_q - z_w, zero padded;
    * ``corr`` int32 [N]: (off_x - z_x) * sum_k w8[n, k] (the device reads x as q_x - off_x);
    * ``mult`` f32 [N]: s_x * s_w[n] * alpha, formed in float64 and rounded once;
    * ``bias`` f32 [N] (zeros when the layer has none).

    With them acc[m, n] = sum_k (q_x - off_x) w8[n, k] gives the layer's value as
    float(acc + corr[n]) * mult[n] + bias[n]."""
    import torch
    n, k = s.wq_np.shape
    if k > Q_MAX_K:
        raise PlanError(f"quantised dense layer: K = {k} exceeds {Q_MAX_K} (the int32 accumulator bound)")
    wq = s.wq_np.astype(np.int64)
    if wq.min(initial=0) < -128 or wq.max(initial=0) > 127:
        raise PlanError("quantised dense layer: w_q - z_w leaves [-128, 127]")
    w8 = np.zeros((-(-n // 128) * 128, -(-k // 64) * 64), np.int8)
    w8[:n, :k] = wq
    corr = (Q_OFF[s.x_type] - int(s.x_zp)) * wq.sum(axis=1)
    mult = (np.float64(s.x_scale) * s.w_scale.astype(np.float64) * np.float64(s.alpha)).astype(np.float32)
    bias = np.zeros(n, np.float32) if s.b_np is None else np.ascontiguousarray(s.b_np, np.float32)
    return dict(w8=torch.from_numpy(w8), corr=torch.from_numpy(corr.astype(np.int32)),
                mult=torch.from_numpy(np.array(np.broadcast_to(mult, (n,)))), bias=torch.from_numpy(np.array(bias)))


def step_inputs(steps, i: int) -> Tuple[int, ...]:
    """Indices of the steps whose outputs step ``i`` reads (-1: the model input)."""
    s = steps[i]
    if s.kind == "join":
        return (s.a, s.b)
    src = getattr(s, "src", None)
    src = i - 1 if src is None else src
    if s.kind == "conv" and s.res is not None:
        return (src, s.res)
    return (src,)


def step_consumers(steps) -> List[List[int]]:
    cons: List[List[int]] = [[] for _ in steps]
    for i in range(len(steps)):
        for j in step_inputs(steps, i):
            if j >= 0:
                cons[j].append(i)
    return cons


@dataclass
class _Val:
    """A graph value during lowering: the step producing it plus what is still pending on it."""
    step: int                 # producing step (-1: the model input)
    width: int                # columns (-1: unknown, a symbolic model input)
    scale: Optional[np.ndarray] = None   # pending per-column affine x * scale + shift (Scaler,
    shift: Optional[np.ndarray] = None   # Add / Sub / Mul / Div by a constant), folded into a neighbour
    exclusive: bool = True    # derived from the step's output through single-use values only
    ml_col: int = 0           # model-score column of the value on the device
    cpu_col: int = 0          # ... and in the CPU executor's output of the same value
    narrowed: bool = False    # a binary classifier lowered to its positive column only
    label: bool = False       # a classifier's label output (not lowered)
    gru_y: bool = False       # a GRU's / LSTM's per-step outputs Y (only another such layer reads them)
    bidir_pending: bool = False  # a layout-0 bidirectional Y_h still in [D, N, H] order
    # QDQ: a QuantizeLinear output (the step's buffer holds the bytes) ...
    quant: Optional[Tuple[np.float32, int, str]] = None   # (scale, zero point, type)
    # ... and a DequantizeLinear of one, not yet materialised: a quantised Gemm reads the bytes of
    # ``step`` directly, any other reader gets a DequantStep first
    deq: Optional[Tuple[np.float32, int, str]] = None
    # a pending column view: one ColRec per column of this value, each a function of one column of
    # the base value (``step``'s output, ``base_width`` columns wide); materialised as a ColumnStep
    # by the first reader that is no column operator
    cols: Optional[List["ColRec"]] = None
    base_width: int = -1
    onehot3d: bool = False    # a OneHotEncoder output still shaped [N, C, n_cats] (Flatten / Reshape next)
    int_cast: bool = False    # behind a Cast to an integer type: only a OneHotEncoder reads it
    rank1: bool = False       # a Gather with a scalar index: [N]
    pool3d: bool = False      # a pooled sequence value still shaped [N, C, 1] (Flatten / Squeeze / Reshape next)


@dataclass
class _Seq:
    """A sequence value during lowering, logically [N, C, T]: the window [off, off + length) of the
    output of ``step`` (-1: the transposed model input), which is zero outside [0, T). ``pending``: the
    window of a convolution whose padding is still being composed (its Slice may follow)."""
    step: int
    C: int
    off: int
    length: int
    pending: bool = False
    exclusive: bool = True


ALIAS_OPS = ("Identity", "Flatten", "Squeeze", "Unsqueeze", "Reshape", "ZipMap", "Cast", "Dropout")
ACT_OPS = ("Relu", "Sigmoid", "Tanh")
# activations that always run as a RowStep: op -> (row act, (attribute, ONNX default) of p0 / p1)
ROW_ACT_OPS = {"LeakyRelu": ("leaky_relu", ("alpha", 0.01), None), "Elu": ("elu", ("alpha", 1.0), None),
               "Selu": ("selu", ("alpha", 1.67326319217681884765625), ("gamma", 1.05070102214813232421875)),
               "Softplus": ("softplus", None, None), "HardSigmoid": ("hard_sigmoid", ("alpha", 0.2), ("beta", 0.5)),
               "Gelu": ("gelu", None, None)}
LINEAR_POST = {"NONE": "none", "LOGISTIC": "sigmoid"}


def compile_onnx(model, input_name: str = "input", output_name: str = "output",
                 depth_limit: int = 12, fuse_heads: bool = True) -> Plan:
    """``model``: _native.OnnxModel. Returns a host-side Plan (upload with :func:`to_device`).

    The nodes the primary output depends on are lowered in dependency order; each value is
    tracked as (producing step, pending affine). Linear ops fold into their neighbours:
    Scaler / constant Add, Sub, Mul, Div into the next dense layer's weights (or the previous
    one's, when it has no activation), a constant Add after MatMul into its bias, Relu /
    Sigmoid / Tanh into the dense epilogue. Two branches meet in a :class:`JoinStep`."""
    N = native()
    try:
        ex = N.Executor(model)
    except RuntimeError as e:   # a malformed or out-of-scope kernel machine: the reader's message
        if str(e).startswith("SVM"):
            raise PlanError(str(e)) from e
        raise
    nodes = model.nodes()
    index = {id(n): i for i, n in enumerate(nodes)}
    inputs = {v[0]: v for v in model.inputs()}
    if input_name not in inputs:
        if len(inputs) == 1:
            input_name = next(iter(inputs))
        else:
            raise PlanError(f"model has no input named {input_name!r}")
    outs = [v[0] for v in model.outputs()]
    if output_name not in outs:
        output_name = outs[-1]
    in_vi = inputs[input_name]
    dims = in_vi[2]
    seq_input = len(dims) == 3
    in_width = int(dims[-1]) if dims and dims[-1] > 0 else -1
    raw_inits = set(model.initializer_names())
    # constants: the initializers, plus every DequantizeLinear of one (added as it is lowered)
    inits = set(raw_inits)
    fconst: Dict[str, np.ndarray] = {}    # DequantizeLinear(initializer) -> the f32 constant
    qconst: Dict[str, Dict[str, Any]] = {}  # ... and its integer form: d = q - z, scale, axis, type

    def const(name):
        return fconst[name] if name in fconst else model.initializer(name)

    # the nodes the output depends on, in dependency order: a depth-first post-order from the
    # output, so each branch's nodes stay contiguous (a dense layer and the N=1 layer reading it
    # end up adjacent for the head fusion)
    prod = {o: n for n in nodes for o in n["outputs"] if o}
    if output_name not in prod:
        raise PlanError(f"output {output_name!r} is not computed by a node")
    # ONNX sequence_lens (input 4 of GRU / LSTM): lowered when it is a graph input typed
    # tensor(int32) of shape [N]; that name is the one graph input allowed beside the model input
    lens_ok = {n["inputs"][4] for n in nodes
               if n["op_type"] in ("GRU", "LSTM") and len(n["inputs"]) > 4 and n["inputs"][4]}
    lens_ok = {name for name in lens_ok
               if name in inputs and name not in inits and name not in prod and name != input_name
               and int(inputs[name][1]) == ONNX_INT32 and len(inputs[name][2]) == 1}
    lens_seen: List[Optional[str]] = []

    def seq_lens(op: str, ins) -> bool:
        """Whether this GRU / LSTM node is masked; every layer of the chain must agree."""
        name = ins[4] if len(ins) > 4 and ins[4] else None
        if name is not None and name not in lens_ok:
            raise PlanError(f"{op}: sequence_lens is lowered only as an int32 graph input of shape [N] "
                            f"({name!r} is not)")
        if lens_seen and lens_seen[0] != name:
            raise PlanError(f"{op}: every layer must read the same sequence_lens input "
                            f"({lens_seen[0]!r} and {name!r})")
        lens_seen.append(name)
        return name is not None
    order, live = [], set()
    stack = [(prod[output_name], 0)]
    while stack:
        n, k = stack.pop()
        if id(n) in live:
            continue
        if k < len(n["inputs"]):
            stack.append((n, k + 1))
            name = n["inputs"][k]
            p = prod.get(name)
            if p is not None and id(p) not in live:
                stack.append((p, 0))
            elif p is None and name and name not in inits and name != input_name and not (
                    k == 4 and n["op_type"] in ("GRU", "LSTM") and name in lens_ok):
                if k == 4 and n["op_type"] in ("GRU", "LSTM"):
                    raise PlanError(f"{n['op_type']}: sequence_lens is lowered only as an int32 graph input of "
                                    f"shape [N] ({name!r} is not)")
                raise PlanError(f"the output depends on graph input {name!r} besides the model input")
            continue
        live.add(id(n))
        order.append(n)

    def root(name):  # the value an alias chain (Identity / Reshape / ZipMap ...) starts from
        n = prod.get(name)
        while n is not None and id(n) in live and n["op_type"] in ALIAS_OPS:
            name = n["inputs"][0]
            n = prod.get(name)
        return name

    uses: Dict[str, int] = {}
    for n in order:
        if n["op_type"] in ALIAS_OPS:
            continue
        for i in set(n["inputs"]):
            if i and i not in inits:
                uses[root(i)] = uses.get(root(i), 0) + 1
    uses[root(output_name)] = uses.get(root(output_name), 0) + 1

    def single_use(name):
        return uses.get(root(name), 0) == 1

    # every name a live node (or the output) reads, unaliased: a node's secondary outputs
    # (a Dropout mask, LayerNormalization's Mean / InvStdDev) are refused when they are in here
    reads = {i for n in order for i in n["inputs"] if i} | {output_name}

    steps: List[Any] = []
    vals: Dict[str, _Val] = {input_name: _Val(-1, in_width)}

    def emit(step, src: int) -> int:
        if step.kind != "join":
            step.src = src
        steps.append(step)
        return len(steps) - 1

    def get(name, what, rank1_ok=False):
        v = vals.get(name)
        if v is None:
            raise PlanError(f"{what}: value {name!r} is not computed by a lowered node")
        if v.label:
            raise PlanError(f"{what}: a classifier's label output is not lowered (the device computes scores)")
        if v.narrowed:
            raise PlanError(f"{what}: reads a binary classifier's scores (lowered to the positive column)")
        if v.gru_y:
            cell = steps[v.step].kind.upper()
            raise PlanError(f"{what}: a {cell}'s per-step outputs are lowered only into another {cell} layer")
        if v.quant is not None:
            raise PlanError(f"{what}: a quantised tensor is read only by DequantizeLinear")
        if v.pool3d:
            raise PlanError(f"{what}: a pooled sequence value [N, C, 1] must be flattened to [N, C] (Flatten / Squeeze / "
                            "Reshape) before anything else reads it")
        if v.deq is not None:   # a reader other than a quantised Gemm: the DequantizeLinear runs on its own
            i = emit(DequantStep(v.width, *v.deq), v.step)
            v = vals[name] = _Val(i, v.width, ml_col=v.ml_col, cpu_col=v.cpu_col)
        if v.cols is not None:  # a reader that is no column operator: the view becomes a step
            v = vals[name] = materialise(v, what, rank1_ok)
        return v

    materialised: Dict[int, Tuple[_Val, _Val]] = {}   # id(view) -> (the view, kept alive; its plain value)

    def materialise(v: _Val, what, rank1_ok=False, int_ok=False) -> _Val:
        """The plain value of a column view: a ColumnStep on its base, or the base itself when the
        view is the identity over all of its columns."""
        if v.onehot3d:
            raise PlanError(f"{what}: a OneHotEncoder output [N, C, n_cats] must be flattened to [N, C * n_cats] "
                            "(Flatten axis 1 / Reshape) before anything else reads it")
        if v.int_cast and not int_ok:
            raise PlanError(f"{what}: Cast to a non-float type is lowered only as the link to a OneHotEncoder")
        if v.rank1 and not rank1_ok:
            raise PlanError(f"{what}: a Gather with a scalar index ([N]) is lowered only into alias ops, Concat "
                            "and FeatureVectorizer")
        if id(v) in materialised:
            return materialised[id(v)][1]
        recs = v.cols
        if v.base_width == len(recs) and all(r.identity and r.src == j for j, r in enumerate(recs)):
            nv = _Val(v.step, len(recs), exclusive=v.exclusive, ml_col=v.ml_col, cpu_col=v.cpu_col)
        else:
            if v.base_width <= 0:
                raise PlanError(f"{what}: column operators on a value of unknown width")
            if v.base_width > COL_MAX_IN:
                raise PlanError(f"{what}: column operators on {v.base_width} columns (> {COL_MAX_IN}) are CPU-only")
            if not 1 <= len(recs) <= COL_MAX_OUT:
                raise PlanError(f"{what}: column operators assemble {len(recs)} columns (1 .. {COL_MAX_OUT} on the device)")
            nv = _Val(emit(ColumnStep(in_width=v.base_width, out_width=len(recs), records=list(recs)), v.step), len(recs))
        materialised[id(v)] = (v, nv)
        return nv

    def plain(name, what) -> _Val:
        """The value with its pending affine applied: folded into the producing dense layer when
        that has no activation and nothing else reads its output, else one diagonal layer."""
        v = get(name, what)
        if v.scale is None:
            return v
        w = v.width if v.width > 0 else max(len(v.scale), len(v.shift))
        if w <= 1 and v.width <= 0:
            raise PlanError(f"{what}: scaling of a value of unknown width")
        sc = np.broadcast_to(v.scale, (w,)).astype(np.float64)
        sh = np.broadcast_to(v.shift, (w,)).astype(np.float64)
        st = steps[v.step] if v.step >= 0 else None
        if st is not None and st.kind == "dense" and st.act == "none" and v.exclusive:
            st.w_np = np.ascontiguousarray(st.w_np * sc[:, None], np.float32)
            b = np.zeros(st.n) if st.b_np is None else st.b_np.astype(np.float64)
            st.b_np = (b * sc + sh).astype(np.float32)
            nv = _Val(v.step, w, ml_col=v.ml_col, cpu_col=v.cpu_col)
        elif st is not None and st.kind == "svm" and st.act == "none" and v.exclusive and w == 1:
            # a constant Mul / Add / Neg on a kernel machine's value: its epilogue
            st.post_scale, st.post_shift = st.post_scale * sc[0], st.post_shift * sc[0] + sh[0]
            nv = _Val(v.step, w, ml_col=v.ml_col, cpu_col=v.cpu_col)
        else:
            i = emit(DenseStep(n=w, k=w, act="none", w_np=np.diag(sc).astype(np.float32),
                               b_np=sh.astype(np.float32)), v.step)
            nv = _Val(i, w)
        vals[name] = nv
        return nv

    def linear(name, w, b, what):
        """(step, w, b) of ``x @ w + b`` for x = ``name`` (w [K, N]): x's pending affine is
        folded into w / b (scale rows of w, shift through w into b)."""
        v = get(name, what)
        if v.width > 0 and w.shape[0] != v.width:
            raise PlanError(f"{what}: weight rows {w.shape[0]} != input width {v.width}")
        if v.scale is not None:
            K = w.shape[0]
            sc = np.broadcast_to(v.scale, (K,)).astype(np.float64)
            sh = np.broadcast_to(v.shift, (K,)).astype(np.float64)
            b64 = (np.zeros(w.shape[1]) if b is None else b.astype(np.float64)) + sh @ w.astype(np.float64)
            w = (sc[:, None] * w.astype(np.float64)).astype(np.float32)
            b = b64.astype(np.float32)
        return v.step, w, b

    def affine(name, out, what, scale=None, shift=None):
        v = get(name, what)
        s0 = np.ones(1) if v.scale is None else v.scale
        t0 = np.zeros(1) if v.shift is None else v.shift
        sc = np.ones(1) if scale is None else np.asarray(scale, np.float64).ravel()
        sh = np.zeros(1) if shift is None else np.asarray(shift, np.float64).ravel()
        w = v.width
        for x in (s0, t0, sc, sh):
            if len(x) > 1:
                if w > 0 and len(x) != w:
                    raise PlanError(f"{what}: {len(x)} per-column constants for width {w}")
                w = len(x)
        vals[out] = replace(v, width=w, scale=s0 * sc, shift=t0 * sc + sh,
                            exclusive=v.exclusive and single_use(name))

    def row_act(name, out, what, act, p0=0.0, p1=0.0, gamma=None):
        """An elementwise activation as a step of its own (rowops.hip) on ``name``'s plain value."""
        v = plain(name, what)
        if v.width <= 0:
            raise PlanError(f"{what}: the width of its input must be known")
        i = emit(RowStep("act", v.width, act=act, p0=float(p0), p1=float(p1), gamma_np=gamma), v.step)
        vals[out] = _Val(i, v.width, ml_col=v.ml_col, cpu_col=v.cpu_col)

    def identity_view(v: _Val) -> _Val:
        return replace(v, cols=[ColRec(j) for j in range(v.width)], base_width=v.width)

    def view(name, what, int_ok=False, rank1_ok=False) -> _Val:
        """The value as a column view (an identity view starts on a plain value)."""
        v = vals.get(name)
        if v is None or v.cols is None:
            v = plain(name, what)
            if v.width <= 0:
                raise PlanError(f"{what}: column operators on a value of unknown width")
            return replace(identity_view(v), exclusive=v.exclusive and single_use(name))
        if v.onehot3d or (v.int_cast and not int_ok) or (v.rank1 and not rank1_ok):
            materialise(v, what)   # raises the matching refusal
        return v

    def fill(name, out, what, v, fits, stage):
        """A per-column operator on the view ``v`` of ``name``: ``stage(rec, column)`` fills the next
        free stage of every record. Where one does not fit (``fits(rec)``), the view is materialised
        first and a fresh identity view starts on the result, so float arithmetic is never reordered."""
        if not all(fits(r) for r in v.cols):
            base = materialise(v, what, rank1_ok=True, int_ok=True)   # the float view behind a pending Cast
            v = replace(identity_view(base), int_cast=v.int_cast, rank1=v.rank1)
        vals[out] = replace(v, cols=[stage(r, j) for j, r in enumerate(v.cols)],
                            exclusive=v.exclusive and single_use(name))

    def select(name, out, what, idx, rank1=False):
        v = view(name, what)
        vals[out] = replace(v, cols=[v.cols[j] for j in idx], width=len(idx), rank1=rank1,
                            exclusive=v.exclusive and single_use(name))

    def int_indices(what, which, name, C, wrap):
        """A constant integer index tensor of ``what`` (ONNX int32 / int64), checked against C columns."""
        if not name or name not in raw_inits:
            raise PlanError(f"{what}: {which} must be a constant (an initializer)")
        if int(model.initializer_dtype(name)) not in ((6, 7) if wrap else (7,)):
            raise PlanError(f"{what}: {which} must be an {'int32 / ' if wrap else ''}int64 tensor")
        arr = np.asarray(model.initializer(name), np.int64)
        idx = [int(j) for j in arr.ravel()]
        for j in idx:
            if not (-C if wrap else 0) <= j < C:
                raise PlanError(f"{what}: index {j} outside the {C} columns")
        return [j + C if j < 0 else j for j in idx], arr.ndim

    def per_column(what, arr, C, name):
        arr = np.asarray(arr, np.float32).ravel()
        if arr.size not in (1, C):
            raise PlanError(f"{what}: {arr.size} values in {name} for {C} columns (1 or one per column)")
        return np.broadcast_to(arr, (C,))

    # ---- sequence values of a temporal-convolution model: [N, C, T], entered through a Transpose of
    # the 3-D model input; every operator on one is lowered in lower_seq below
    seqs: Dict[str, _Seq] = {}
    sq = dict(T=0, layout=0)

    def ints_of(what, which, name):
        if not name or name not in raw_inits or int(model.initializer_dtype(name)) not in (6, 7):
            raise PlanError(f"{what}: {which} must be a constant integer tensor (an initializer)")
        return [int(j) for j in np.asarray(model.initializer(name), np.int64).ravel()]

    def seq_value(name) -> _Seq:
        """The value as any reader but a Slice sees it: a convolution's composed padding is fixed now."""
        v, T = seqs[name], sq["T"]
        if v.pending:
            st = steps[v.step]
            span = st.dil * (st.k - 1)
            if not v.exclusive:
                raise PlanError("Conv: its padded output is cut by a Slice and also read elsewhere; one layer has one "
                                "left padding, so several cuts of one convolution are not lowered")
            if v.length != T:
                raise PlanError(f"Conv: its padded and cut output has length {v.length}, not T = {T} "
                                "(a convolution layer of a sequence model keeps the length)")
            if not 0 <= -v.off <= span:
                raise PlanError(f"Conv: pads and cuts compose to a left padding of {-v.off}, outside "
                                f"[0, d (k - 1) = {span}]")
            st.pad_left = -v.off
            v = seqs[name] = replace(v, off=0, pending=False)
        return v

    def seq_full(name, what) -> _Seq:
        v = seq_value(name)
        if v.off != 0 or v.length != sq["T"]:
            raise PlanError(f"{what}: reads a padded or cut sequence value (steps [{v.off}, {v.off + v.length}) of "
                            f"T = {sq['T']}); only a Conv or a Slice may follow a Pad or a Slice")
        return v

    def seq_covers(v: _Seq, what):
        if v.off > 0 or v.off + v.length < sq["T"]:
            raise PlanError(f"{what}: reads a sequence value cut inside its T steps (steps [{v.off}, "
                            f"{v.off + v.length}) of {sq['T']}): the cut is not lowered")

    def seq_pool(opname, v, out_, what, keep3d):
        if v.step < 0:
            raise PlanError(f"{what}: a read-out of the model input itself is not lowered")
        i = emit(SeqPoolStep(opname, v.C, seq=sq["T"], layout=sq["layout"]), v.step)
        vals[out_] = _Val(i, v.C, pool3d=keep3d)

    def lower_seq(n):
        op, a, ins = n["op_type"], n["attrs"], n["inputs"]
        x_, out_ = ins[0], n["outputs"][0]
        T = sq["T"]
        if x_ not in seqs and op != "Add":
            raise PlanError(f"op {op} with a sequence value as a secondary input is not lowered")
        if op == "Conv":
            if any(s.kind in RECURRENT_KINDS for s in steps):
                raise PlanError("Conv: GRU / LSTM layers and Conv mixed in one model are not lowered")
            v = seq_value(x_)
            seq_covers(v, op)
            if len(ins) < 2 or ins[1] not in inits:
                raise PlanError("Conv: W must be an initializer")
            w = np.asarray(const(ins[1]), np.float32)
            if w.ndim != 3:
                raise PlanError(f"Conv: only 1-D convolutions are lowered (W [M, C, k]; this one has rank {w.ndim})")
            M_, C_, k_ = (int(d_) for d_ in w.shape)
            if int(a.get("group", 1)) != 1:
                raise PlanError(f"Conv: group {int(a.get('group', 1))} is not lowered (1 only)")
            ks = [int(j) for j in a.get("kernel_shape", [k_])]
            dl = [int(j) for j in a.get("dilations", [1])]
            sd = [int(j) for j in a.get("strides", [1])]
            if ks != [k_] or len(dl) != 1 or len(sd) != 1:
                raise PlanError(f"Conv: kernel_shape {ks} / dilations {dl} / strides {sd} do not describe W's 1-D kernel of {k_}")
            if sd != [1]:
                raise PlanError(f"Conv: stride {sd[0]} is not lowered (1 only)")
            d_ = dl[0]
            if d_ < 1 or k_ < 1:
                raise PlanError("Conv: a dilation or kernel size of 0")
            if C_ != v.C:
                raise PlanError(f"Conv: W has {C_} input channels, the value {v.C}")
            b = np.zeros(M_, np.float32)
            if len(ins) > 2 and ins[2]:
                if ins[2] not in inits:
                    raise PlanError("Conv: B must be an initializer")
                b = np.asarray(const(ins[2]), np.float32).ravel()
                if b.size != M_:
                    raise PlanError(f"Conv: B holds {b.size} values for {M_} output channels")
            span = d_ * (k_ - 1)
            ap = str(a.get("auto_pad", "NOTSET"))
            if ap == "NOTSET":
                pads = [int(j) for j in a.get("pads", [0, 0])]
                if len(pads) != 2 or min(pads) < 0:
                    raise PlanError(f"Conv: pads {pads} (two non-negative values [begin, end])")
                cl, cr = pads
            elif ap in ("SAME_UPPER", "SAME_LOWER"):
                cl = span // 2 if ap == "SAME_UPPER" else span - span // 2
                cr = span - cl
            elif ap == "VALID":
                cl = cr = 0
            else:
                raise PlanError(f"Conv: unknown auto_pad {ap!r}")
            st = ConvStep(c_in=C_, c_out=M_, k=k_, dil=d_, pad_left=0, w_np=np.ascontiguousarray(w.transpose(0, 2, 1)),
                          b_np=np.ascontiguousarray(b, np.float32), seq=T, layout=sq["layout"])
            check_conv(st)   # the device limits (the padding is checked when it is fixed)
            seqs[out_] = _Seq(emit(st, v.step), M_, v.off - cl, v.length + cl + cr - span, pending=True)
        elif op == "Pad":
            v = seq_value(x_)
            seq_covers(v, op)
            if str(a.get("mode", "constant")) != "constant":
                raise PlanError(f"Pad: mode {a.get('mode')!r} is not lowered (constant only)")
            if len(ins) > 3 and ins[3]:
                raise PlanError("Pad: the axes input is not lowered")
            if len(ins) > 1 and ins[1]:
                pads = ints_of(op, "pads", ins[1])
                val = 0.0
                if len(ins) > 2 and ins[2]:
                    if ins[2] not in inits:
                        raise PlanError("Pad: the value must be a constant (an initializer)")
                    val = float(np.asarray(const(ins[2]), np.float64).ravel()[0])
            else:
                pads, val = [int(j) for j in a.get("pads", [])], float(a.get("value", 0.0))
            if len(pads) != 6 or min(pads) < 0:
                raise PlanError(f"Pad: pads {pads} on a sequence value (six non-negative values)")
            if val != 0.0:
                raise PlanError(f"Pad: a non-zero pad value ({val:g}) on a sequence value is not lowered")
            if pads[0] or pads[1] or pads[3] or pads[4]:
                raise PlanError("Pad: padding on N or C of a sequence value is not lowered (the time axis only)")
            seqs[out_] = replace(v, off=v.off - pads[2], length=v.length + pads[2] + pads[5],
                                 exclusive=v.exclusive and single_use(x_))
        elif op == "Slice":
            if any(k_ in a for k_ in ("starts", "ends", "axes")):
                raise PlanError("Slice: the attribute form (opset < 10) is not lowered")
            v = seqs[x_]
            starts = ints_of(op, "starts", ins[1] if len(ins) > 1 else "")
            ends = ints_of(op, "ends", ins[2] if len(ins) > 2 else "")
            axes = ints_of(op, "axes", ins[3]) if len(ins) > 3 and ins[3] else list(range(len(starts)))
            stp = ints_of(op, "steps", ins[4]) if len(ins) > 4 and ins[4] else [1] * len(starts)
            if not len(starts) == len(ends) == len(axes) == len(stp):
                raise PlanError("Slice: starts, ends, axes and steps differ in length")
            off, length, cut = v.off, v.length, False
            for s_, e_, ax, st_ in zip(starts, ends, axes, stp):
                ax += 3 if ax < 0 else 0
                if ax not in (0, 1, 2):
                    raise PlanError(f"Slice: axis {ax} of a sequence value [N, C, T]")
                if st_ != 1:
                    raise PlanError(f"Slice: a cut that is not contiguous (step {st_}) on a sequence value is not lowered")
                if ax != 2:   # N is symbolic, C known: the explicit full range only
                    if s_ != 0 or e_ < (2 ** 31 - 1 if ax == 0 else v.C):
                        raise PlanError("Slice: only the time axis of a sequence value may be cut (N and C keep their "
                                        "full range)")
                    continue
                if cut:
                    raise PlanError("Slice: the time axis is named twice")
                cut = True
                s_, e_ = (s_ + length if s_ < 0 else s_), (e_ + length if e_ < 0 else e_)
                s_, e_ = min(max(s_, 0), length), min(max(e_, 0), length)
                if e_ <= s_:
                    raise PlanError("Slice: an empty cut of a sequence value")
                if (v.pending and 1 < T == length and (s_, e_) == (T - 1, T)
                        and 0 <= -off <= steps[v.step].dil * (steps[v.step].k - 1)):
                    # the last step of a convolution whose padding already composes (no activation in
                    # between): a read-out, not part of the padding; the layer is fixed first
                    v = seq_value(x_)
                    off, length = v.off, v.length
                off, length = off + s_, e_ - s_
            seqs[out_] = replace(v, off=off, length=length, exclusive=v.exclusive and single_use(x_))
        elif op in ACT_OPS:
            v = seq_full(x_, op)
            st = steps[v.step] if v.step >= 0 else None
            ok = st is not None and st.kind == "conv" and v.exclusive and single_use(x_)
            if ok and st.res is None and st.act == "none" and st.act_post == "none":
                st.act = op.lower()
            elif ok and st.act_post == "none":
                st.act_post = op.lower()
            else:
                raise PlanError(f"{op}: an activation on a sequence value folds only into the convolution producing it "
                                "(this value has several readers, is the model input, or both activation slots of "
                                "the layer are taken)")
            seqs[out_] = replace(v)
        elif op == "Add":
            if len(ins) != 2 or any(i not in seqs for i in ins):
                raise PlanError("Add: on a sequence value only the sum of two sequence values (a residual connection) is lowered")
            va, vb = seq_full(ins[0], op), seq_full(ins[1], op)
            if va.C != vb.C:
                raise PlanError(f"Add: sequence values of {va.C} and {vb.C} channels")
            best = None
            for v, name, o in ((va, ins[0], vb), (vb, ins[1], va)):
                st = steps[v.step] if v.step >= 0 else None
                if (st is not None and st.kind == "conv" and st.res is None and st.act_post == "none" and v.exclusive
                        and single_use(name) and 0 <= o.step < v.step and (best is None or v.step > best[0].step)):
                    best = (v, o)
            if best is None:
                raise PlanError("Add: a residual Add folds into a convolution whose output has no other reader; the "
                                "other operand must be computed before it, by a step (not the model input)")
            steps[best[0].step].res = best[1].step
            seqs[out_] = _Seq(best[0].step, va.C, 0, T)
        elif op == "BatchNormalization":
            v = seqs[x_]
            if int(a.get("training_mode", 0)):
                raise PlanError("BatchNormalization: training_mode=1 is not lowered (inference only)")
            if len(ins) < 5 or any(i not in inits for i in ins[1:5]):
                raise PlanError("BatchNormalization: scale, B, mean and var must be initializers")
            if any(o and o in reads for o in n["outputs"][1:]):
                raise PlanError("BatchNormalization: the running statistics outputs are not lowered")
            st = steps[v.step] if v.step >= 0 else None
            if not (st is not None and st.kind == "conv" and st.act == "none" and st.res is None and st.act_post == "none"
                    and v.exclusive and single_use(x_)):
                raise PlanError("BatchNormalization: on a sequence value it folds only into the convolution producing "
                                "it (before its activation, no other reader)")
            g_, b_, mu, var = (np.asarray(const(i), np.float64).ravel() for i in ins[1:5])
            if not g_.size == b_.size == mu.size == var.size == v.C:
                raise PlanError(f"BatchNormalization: scale / B / mean / var must hold one value per channel ({v.C})")
            sc = g_ / np.sqrt(var + float(a.get("epsilon", 1e-5)))
            st.w_np = np.ascontiguousarray(st.w_np.astype(np.float64) * sc[:, None, None], np.float32)
            st.b_np = (st.b_np.astype(np.float64) * sc + (b_ - mu * sc)).astype(np.float32)
            seqs[out_] = replace(v)
        elif op in ("Identity", "Dropout"):
            if op == "Dropout":
                if len(n["outputs"]) > 1 and n["outputs"][1] and n["outputs"][1] in reads:
                    raise PlanError("Dropout: its mask output is read, which is not lowered")
                if len(ins) > 2 and ins[2] in inits and np.asarray(const(ins[2])).ravel()[:1].any():
                    raise PlanError("Dropout: training_mode is a constant true (inference only)")
            seqs[out_] = seqs[x_]
        elif op in ("GlobalAveragePool", "GlobalMaxPool"):
            seq_pool("mean" if op == "GlobalAveragePool" else "max", seq_full(x_, op), out_, op, True)
        elif op in ("ReduceMean", "ReduceMax", "ReduceSum"):
            axes = (ints_of(op, "axes", ins[1]) if len(ins) > 1 and ins[1] else [int(j) for j in a.get("axes", [])])
            if [ax + 3 if ax < 0 else ax for ax in axes] != [2]:
                raise PlanError(f"{op}: on a sequence value only a reduction over the time axis (axis 2) alone is lowered")
            seq_pool(op[6:].lower(), seq_full(x_, op), out_, op, bool(int(a.get("keepdims", 1))))
        elif op == "Gather":
            if int(a.get("axis", 0)) not in (2, -1):
                raise PlanError(f"Gather: axis {int(a.get('axis', 0))} of a sequence value is not lowered (the time axis only)")
            idx = ints_of(op, "the indices", ins[1] if len(ins) > 1 else "")
            nd = np.asarray(model.initializer(ins[1])).ndim
            if nd > 1 or len(idx) != 1 or idx[0] not in (-1, T - 1):
                raise PlanError("Gather: on a sequence value only the last step (index -1 or T - 1) is lowered")
            seq_pool("last", seq_full(x_, op), out_, op, nd == 1)
        elif op in ("Squeeze", "Flatten", "Reshape"):
            v = seq_value(x_)
            if v.off != T - 1 or v.length != 1:
                raise PlanError(f"{op}: on a sequence value it is lowered only behind a Slice of the last step ([T - 1 : T])")
            seq_pool("last", v, out_, op, False)
        else:
            raise PlanError(f"op {op} is not lowered on a sequence value ([N, C, T]: Conv, Pad, Slice, Relu / Sigmoid / "
                            "Tanh, a residual Add, BatchNormalization, Dropout, Identity and the read-outs are)")

    for n in order:
        op, a = n["op_type"], n["attrs"]
        ins = n["inputs"]
        x = ins[0] if ins else ""
        if op == "Transpose" and x == input_name and seq_input and not seqs:
            perm = [int(p) for p in a.get("perm", [])]
            if perm in ([1, 2, 0], [0, 2, 1]):
                lay = 0 if perm == [1, 2, 0] else 1
                T_ = int(dims[1] if lay else dims[0])
                if in_width <= 0 or T_ <= 0:
                    raise PlanError("Transpose: a temporal-convolution model needs fixed seq and feature dimensions of its input")
                if T_ > CONV_MAX_T:
                    raise PlanError(f"conv: {T_} time steps (the device kernel takes 1 .. {CONV_MAX_T})")
                sq["T"], sq["layout"] = T_, lay
                seqs[n["outputs"][0]] = _Seq(-1, in_width, 0, T_)
                continue
        if any(i in seqs for i in ins):
            lower_seq(n)
            continue
        if op in ("GRU", "LSTM") and any(s.kind in ("conv", "seqpool") for s in steps):
            raise PlanError(f"{op}: GRU / LSTM layers and Conv mixed in one model are not lowered")
        if op in ("QLinearMatMul", "QLinearConv", "QLinearAdd", "QGemm", "MatMulInteger", "ConvInteger",
                  "DynamicQuantizeLinear"):
            raise PlanError(f"op {op} is not lowered to the device: {QDQ_ONLY}")
        if op in ("QuantizeLinear", "DequantizeLinear"):
            out = n["outputs"][0]
            if int(a.get("block_size", 0)):
                raise PlanError(f"{op}: block_size (blocked quantisation) is not lowered")
            if int(a.get("saturate", 1)) != 1:
                raise PlanError(f"{op}: saturate=0 is not lowered")
            od = int(a.get("output_dtype", 0))
            if od not in (0, ONNX_UINT8, ONNX_INT8):
                raise PlanError(f"{op}: output_dtype {od} is not lowered (uint8 and int8 only)")
            has_zp = len(ins) > 2 and bool(ins[2])
            if len(ins) < 2 or ins[1] not in raw_inits or (has_zp and ins[2] not in raw_inits):
                raise PlanError(f"{op}: scale and zero point must be constants (initializers)")
            if int(model.initializer_dtype(ins[1])) != 1:
                raise PlanError(f"{op}: the scale must be a float32 tensor")
            sc = np.asarray(model.initializer(ins[1]), np.float32).ravel()
            zp = np.asarray(model.initializer(ins[2]), np.int64).ravel() if has_zp else np.zeros(sc.size, np.int64)
            zt = int(model.initializer_dtype(ins[2])) if has_zp else 0
            if zp.size != sc.size or sc.size < 1 or not (sc > 0).all():
                raise PlanError(f"{op}: scale (positive) and zero point must have the same size")
            if op == "DequantizeLinear" and x in raw_inits:
                # a constant: int8 / uint8 weights, an int32 bias; per-axis scales allowed
                xt = int(model.initializer_dtype(x))
                if xt not in (ONNX_UINT8, ONNX_INT8, ONNX_INT32):
                    raise PlanError(f"DequantizeLinear: a constant of ONNX type {xt} is not lowered (uint8, int8, int32)")
                if has_zp and zt != xt:
                    raise PlanError("DequantizeLinear: the zero point's type differs from the tensor's")
                q = np.asarray(model.initializer(x), np.int64)
                axis, shape = None, [1] * q.ndim
                if sc.size != 1:
                    axis = int(a.get("axis", 1))
                    axis += q.ndim if axis < 0 else 0
                    if not 0 <= axis < q.ndim or q.shape[axis] != sc.size:
                        raise PlanError(f"DequantizeLinear: {sc.size} scales do not match axis {axis} of shape {q.shape}")
                    shape[axis] = sc.size
                d = q - zp.reshape(shape)
                fconst[out] = (d.astype(np.float64) * sc.astype(np.float64).reshape(shape)).astype(np.float32)
                qconst[out] = dict(d=d, scale=sc, axis=axis, xt=xt)
                inits.add(out)
                continue
            if sc.size != 1:
                raise PlanError(f"{op}: per-axis quantisation of activations is not lowered")
            if op == "QuantizeLinear":
                qt = QTYPES.get(zt if has_zp else (od or ONNX_UINT8))
                if qt is None or (od and has_zp and od != zt):
                    raise PlanError(f"QuantizeLinear: zero point of ONNX type {zt} is not lowered (uint8 and int8 only)")
                if not Q_RANGE[qt][0] <= int(zp[0]) <= Q_RANGE[qt][1]:
                    raise PlanError("QuantizeLinear: the zero point lies outside its type")
                v = plain(x, op)
                if v.width <= 0:
                    raise PlanError("QuantizeLinear: the width of its input must be known")
                qi = (sc[0], int(zp[0]), qt)
                st = steps[v.step] if v.step >= 0 else None
                if (st is not None and st.kind == "qdense" and st.out_q is None and v.exclusive and single_use(x)):
                    st.out_q, idx = qi, v.step    # requantisation in the layer's epilogue
                else:   # at the model input, after a tree / join / row op, or on a value with other readers
                    idx = emit(QuantStep(v.width, *qi), v.step)
                vals[out] = _Val(idx, v.width, ml_col=v.ml_col, cpu_col=v.cpu_col, quant=qi)
                continue
            v = vals.get(x)
            if v is None or v.quant is None:
                raise PlanError("DequantizeLinear: lowered on an initializer or on a QuantizeLinear output")
            if has_zp and QTYPES.get(zt) != v.quant[2]:
                raise PlanError("DequantizeLinear: the zero point's type differs from the quantised tensor's")
            if not Q_RANGE[v.quant[2]][0] <= int(zp[0]) <= Q_RANGE[v.quant[2]][1]:
                raise PlanError("DequantizeLinear: the zero point lies outside its type")
            vals[out] = _Val(v.step, v.width, ml_col=v.ml_col, cpu_col=v.cpu_col, deq=(sc[0], int(zp[0]), v.quant[2]))
            continue
        if op in ("Gemm", "MatMul") and len(ins) > 1 and ins[1] in qconst and x in vals and vals[x].deq is not None:
            qc, v = qconst[ins[1]], vals[x]
            tb = op == "Gemm" and bool(int(a.get("transB", 0)))
            if op == "Gemm" and int(a.get("transA", 0)):
                raise PlanError("Gemm transA=1 is not lowered")
            # a scale per output channel (or one): anything else runs as a float layer on the dequantised weight
            if qc["xt"] in QTYPES and qc["d"].ndim == 2 and qc["axis"] in (None, 0 if tb else 1):
                d = qc["d"] if tb else qc["d"].T                    # [N, K]
                N_, K_ = int(d.shape[0]), int(d.shape[1])
                if v.width > 0 and K_ != v.width:
                    raise PlanError(f"{op}: weight rows {K_} != input width {v.width}")
                if d.min(initial=0) < -128 or d.max(initial=0) > 127:
                    raise PlanError(f"{op}: the quantised weight minus its zero point leaves [-128, 127]")
                if K_ > Q_MAX_K:
                    raise PlanError(f"{op}: a quantised layer with K = {K_} > {Q_MAX_K} is not lowered")
                alpha = float(a.get("alpha", 1.0)) if op == "Gemm" else 1.0
                b = None
                if op == "Gemm" and len(ins) > 2 and ins[2]:
                    if ins[2] not in inits:
                        raise PlanError("Gemm: bias must be an initializer (or a DequantizeLinear of one)")
                    b = np.asarray(const(ins[2]), np.float32).ravel() * np.float32(a.get("beta", 1.0))
                    if b.size == 1 and N_ > 1:
                        b = np.full(N_, b[0], np.float32)
                    if b.size != N_:
                        raise PlanError("Gemm: bias length differs from the output width")
                wf = fconst[ins[1]] if tb else fconst[ins[1]].T
                idx = emit(QDenseStep(n=N_, k=K_, act="none", wq_np=np.ascontiguousarray(d, np.int32),
                                      w_scale=np.ascontiguousarray(np.broadcast_to(qc["scale"], (N_,)), np.float32),
                                      alpha=alpha, x_scale=v.deq[0], x_zp=v.deq[1], x_type=v.deq[2],
                                      w_np=np.ascontiguousarray(wf * np.float32(alpha), np.float32), b_np=b), v.step)
                vals[n["outputs"][0]] = _Val(idx, N_)
                continue
        if op in ("TreeEnsembleClassifier", "TreeEnsembleRegressor", "TreeEnsemble"):
            # the opset-5 TreeEnsemble compiles to the same Ensemble (no label output, no base values)
            v = plain(x, op)
            info = ex.tree_info(index[id(n)])
            if int(info["k"]) > SPARSE_MAX_K:
                raise PlanError(f"TreeEnsemble with {info['k']} targets (> {SPARSE_MAX_K}) is CPU-only")
            layout = choose_tree_layout(info, depth_limit)
            c = (ex.tree_complete(index[id(n)], depth_limit) if layout == "complete"
                 else ex.tree_sparse(index[id(n)]))
            post = int(c["post"])
            binary = bool(c["binary_case"])
            k = int(c["k"])
            n_out = int(c["n_outputs"]) if c["classifier"] else k
            base = np.asarray(c["base_values"], np.float32)
            if binary:
                base = base[:1] if len(base) == 1 else (base[c["binary_class"]:c["binary_class"] + 1]
                                                        if len(base) == 2 else None)
            elif len(base):  # targets past the given base values get 0 (executor semantics)
                base = np.pad(base[:k], (0, max(0, k - len(base))))
            sparse = layout == "sparse"
            ts = TreeStep(n_trees=int(c["n_trees"]), depth=int(c["depth"]), k=k, n_out=n_out, post=post,
                          average=int(c["aggregate"] == 1), binary_class=int(c["binary_class"]) if binary else -1,
                          all_positive=int(bool(c["weights_all_positive"])), max_feature=int(c["max_feature"]),
                          nodes_np=np.ascontiguousarray(c["nodes"], np.int32 if sparse else np.float32),
                          leaves_np=None if sparse else np.ascontiguousarray(c["leaves"], np.float32),
                          base_np=None if base is None or len(base) == 0 else np.asarray(base, np.float32),
                          classifier=bool(c["classifier"]), layout=layout, aggregate=int(c["aggregate"]),
                          roots_np=np.ascontiguousarray(c["roots"], np.int32) if sparse else None,
                          leaf_w_np=np.ascontiguousarray(c["leaf_w"], np.float32) if sparse else None,
                          leaf_has_np=np.ascontiguousarray(c["leaf_has"], np.uint8) if sparse else None,
                          sets_np=np.ascontiguousarray(c["sets"], np.uint32))
            idx = emit(ts, v.step)
            if c["classifier"]:
                col = 1 if n_out == 2 else 0
                vals[n["outputs"][0]] = _Val(idx, 1, label=True)
                if len(n["outputs"]) > 1:
                    vals[n["outputs"][1]] = _Val(idx, n_out, ml_col=col, cpu_col=col)
                else:  # a single output holds the probabilities
                    vals[n["outputs"][0]] = _Val(idx, n_out, ml_col=col, cpu_col=col)
            else:
                vals[n["outputs"][0]] = _Val(idx, k)
            continue
        if op in ("Gemm", "MatMul"):
            if len(ins) < 2 or ins[1] not in inits:
                raise PlanError(f"{op}: weight must be an initializer")
            w = np.asarray(const(ins[1]), np.float32)
            if w.ndim != 2:
                raise PlanError(f"{op}: weight must be 2-D")
            b = None
            if op == "Gemm":
                if int(a.get("transA", 0)):
                    raise PlanError("Gemm transA=1 is not lowered")
                if int(a.get("transB", 0)):
                    w = w.T
                w = w * float(a.get("alpha", 1.0))
                if len(ins) > 2 and ins[2]:
                    if ins[2] not in inits:
                        raise PlanError("Gemm: bias must be an initializer")
                    b = np.asarray(const(ins[2]), np.float32).ravel() * float(a.get("beta", 1.0))
                    if b.size == 1 and w.shape[1] > 1:
                        b = np.full(w.shape[1], b[0], np.float32)
                    if b.size != w.shape[1]:
                        raise PlanError("Gemm: bias length differs from the output width")
            src, w, b = linear(x, w, b, op)
            idx = emit(DenseStep(n=int(w.shape[1]), k=int(w.shape[0]), act="none",
                                 w_np=np.ascontiguousarray(w.T, np.float32), b_np=b), src)
            vals[n["outputs"][0]] = _Val(idx, int(w.shape[1]))
            continue
        if op in ("Add", "Sub", "Mul", "Div"):
            dyn = [i for i in ins if i not in inits]
            if op == "Add" and len(dyn) == 2:
                va, vb = plain(dyn[0], op), plain(dyn[1], op)
                if va.width <= 0 or va.width != vb.width:
                    raise PlanError(f"Add join: widths {va.width} and {vb.width} must be equal and known")
                idx = emit(JoinStep("add", va.step, vb.step, va.width, vb.width), -1)
                vals[n["outputs"][0]] = _Val(idx, va.width)
                continue
            if len(dyn) != 1:
                raise PlanError(f"{op}: only a constant operand or an Add of two branches is lowered")
            xd = dyn[0]
            cst = np.asarray(const([i for i in ins if i != xd][0]), np.float64).ravel()
            first = ins[0] == xd
            v = get(xd, op)
            st = steps[v.step] if v.step >= 0 else None
            if (op == "Add" and v.scale is None and st is not None and st.kind in ("dense", "qdense")
                    and st.act == "none" and getattr(st, "out_q", None) is None
                    and v.exclusive and single_use(xd) and cst.size in (1, st.n)):
                # MatMul + Add (and any constant added to a linear layer): the layer's bias
                b = np.zeros(st.n) if st.b_np is None else st.b_np.astype(np.float64)
                st.b_np = (b + np.broadcast_to(cst, (st.n,))).astype(np.float32)
                vals[n["outputs"][0]] = replace(v)
            elif op == "Add":
                affine(xd, n["outputs"][0], op, shift=cst)
            elif op == "Sub":
                affine(xd, n["outputs"][0], op, shift=-cst) if first else affine(xd, n["outputs"][0], op,
                                                                                  scale=-1.0, shift=cst)
            elif op == "Mul":
                affine(xd, n["outputs"][0], op, scale=cst)
            elif first:
                affine(xd, n["outputs"][0], op, scale=1.0 / cst)
            else:
                raise PlanError("Div of a constant by a value is not lowered")
            continue
        out0 = n["outputs"][0] if n["outputs"] else ""
        if op in ("ArrayFeatureExtractor", "Gather"):
            v = view(x, op)
            if op == "Gather" and int(a.get("axis", 0)) not in (1, -1):
                raise PlanError(f"Gather: axis {int(a.get('axis', 0))} is not lowered (the feature axis of a 2-D value only)")
            idx, nd = int_indices(op, "the indices", ins[1] if len(ins) > 1 else "", v.width, wrap=op == "Gather")
            if op == "Gather" and (nd > 1 or (nd == 0 and len(idx) != 1)):
                raise PlanError("Gather: the indices must be a scalar or 1-D")
            select(x, out0, op, idx, rank1=op == "Gather" and nd == 0)
            continue
        if op == "Slice":
            if any(k in a for k in ("starts", "ends", "axes")):
                raise PlanError("Slice: the attribute form (opset < 10) is not lowered")
            v = view(x, op)
            parts = []
            for k, which in ((1, "starts"), (2, "ends"), (3, "axes"), (4, "steps")):
                name_k = ins[k] if len(ins) > k else ""
                if not name_k and k > 2:
                    parts.append(None)
                    continue
                if name_k not in raw_inits or int(model.initializer_dtype(name_k)) not in (6, 7):
                    raise PlanError(f"Slice: {which} must be a constant integer tensor (an initializer)")
                parts.append([int(j) for j in np.asarray(model.initializer(name_k), np.int64).ravel()])
            starts, ends, axes, steps_ = parts
            axes = list(range(len(starts))) if axes is None else axes
            steps_ = [1] * len(starts) if steps_ is None else steps_
            if not len(starts) == len(ends) == len(axes) == len(steps_):
                raise PlanError("Slice: starts, ends, axes and steps differ in length")
            idx, C, cut = list(range(v.width)), v.width, False
            for s_, e_, ax, st_ in zip(starts, ends, axes, steps_):
                if st_ == 0 or ax not in (0, 1, -1, -2):
                    raise PlanError(f"Slice: step {st_} on axis {ax} of a 2-D value")
                if ax in (0, -2):   # the row axis: N is symbolic, so only the explicit full range
                    if s_ != 0 or st_ != 1 or e_ < 2 ** 31 - 1:
                        raise PlanError("Slice: only the last axis may be cut (axis 0 must keep its full range)")
                    continue
                if cut:
                    raise PlanError("Slice: the last axis is named twice")
                cut = True
                s_, e_ = (s_ + C if s_ < 0 else s_), (e_ + C if e_ < 0 else e_)
                if st_ > 0:
                    idx = list(range(min(max(s_, 0), C), min(max(e_, 0), C), st_))
                else:
                    idx = list(range(min(max(s_, 0), C - 1), min(max(e_, -1), C - 1), st_))
            select(x, out0, op, idx)
            continue
        if op == "Imputer":
            if "imputed_value_int64s" in a or "replaced_value_int64" in a:
                raise PlanError("Imputer: the int64 attributes are not lowered")
            v = view(x, op)
            val = per_column(op, a.get("imputed_value_floats", []), v.width, "imputed_value_floats")
            rep = float(np.float32(a.get("replaced_value_float", 0.0)))
            fill(x, out0, op, v, lambda r: r.identity,
                 lambda r, j: replace(r, imp=(rep, float(val[j]))))
            continue
        if op == "Scaler" and x in vals and vals[x].cols is not None:
            # on a view: the record's affine stage, in the Scaler's own f32 order (no float64 folding)
            v = view(x, op)
            off = per_column(op, a.get("offset", [0.0]), v.width, "offset")
            sc = per_column(op, a.get("scale", [1.0]), v.width, "scale")
            fill(x, out0, op, v, lambda r: r.aff is None and r.mode == "pass",
                 lambda r, j: replace(r, aff=(float(off[j]), float(sc[j]))))
            continue
        if op == "Binarizer":
            v = view(x, op)
            thr = float(np.float32(a.get("threshold", 0.0)))
            fill(x, out0, op, v, lambda r: r.mode == "pass", lambda r, j: replace(r, mode="binarize", arg=thr))
            continue
        if op == "OneHotEncoder":
            if "cats_strings" in a:
                raise PlanError("OneHotEncoder: cats_strings (string categories) is not lowered")
            cats = [int(c) for c in np.asarray(a.get("cats_int64s", []), np.int64).ravel()]
            if not cats:
                raise PlanError("OneHotEncoder: cats_int64s is required")
            if int(a.get("zeros", 1)) == 0:
                raise PlanError("OneHotEncoder: zeros = 0 (an unmatched value is an error) is CPU-only")
            if any(c == -2 ** 63 for c in cats):
                raise PlanError("OneHotEncoder: a category equal to INT64_MIN is not lowered")
            v = view(x, op, int_ok=True, rank1_ok=True)
            if not all(r.mode == "pass" for r in v.cols):
                base = materialise(v, op, rank1_ok=True, int_ok=True)
                v = replace(identity_view(base), rank1=v.rank1)
            # the category as the f32 value it equals; one no f32 represents can never match an f32 input
            f32 = [float(np.float32(c)) for c in cats]
            recs = [replace(r, mode="onehot", arg=f) if int(f) == c else replace(r, mode="zero")
                    for r in v.cols for c, f in zip(cats, f32)]
            vals[out0] = replace(v, cols=recs, width=len(recs), int_cast=False, rank1=False, onehot3d=not v.rank1,
                                 exclusive=v.exclusive and single_use(x))
            continue
        if op in ("Concat", "FeatureVectorizer"):
            vs = [vals.get(i) for i in ins]
            fv_op = op == "FeatureVectorizer"
            if ((fv_op or int(a.get("axis", 0)) in (1, -1)) and vs
                    and all(v is not None and v.cols is not None and not v.onehot3d and not v.int_cast
                            and (fv_op or not v.rank1) for v in vs)
                    and len({v.step for v in vs}) == 1):
                # views over the same base: their records side by side, no step
                if fv_op and "inputdimensions" in a:
                    dims_ = [int(d) for d in np.asarray(a["inputdimensions"]).ravel()]
                    if dims_ != [v.width for v in vs]:
                        raise PlanError(f"FeatureVectorizer: inputdimensions {dims_} differ from the input widths "
                                        f"{[v.width for v in vs]}")
                recs = [r for v in vs for r in v.cols]
                vals[out0] = replace(vs[0], cols=recs, width=len(recs), rank1=False,
                                     exclusive=all(v.exclusive and single_use(i) for v, i in zip(vs, ins)))
                continue
        if op == "FeatureVectorizer":
            # views over different bases, or views beside ordinary values: each is materialised, then
            # the pairwise joins of Concat
            if not ins or any(i in inits for i in ins):
                raise PlanError("FeatureVectorizer is lowered on one or more computed values")
            ws = [get(i, op, rank1_ok=True).width for i in ins]
            if "inputdimensions" in a and [int(d) for d in np.asarray(a["inputdimensions"]).ravel()] != ws:
                raise PlanError(f"FeatureVectorizer: inputdimensions differ from the input widths {ws}")
            acc = plain(ins[0], op)
            for nxt in ins[1:]:
                vb = plain(nxt, op)
                if acc.width <= 0 or vb.width <= 0:
                    raise PlanError("FeatureVectorizer: input widths must be known")
                idx = emit(JoinStep("concat", acc.step, vb.step, acc.width, vb.width), -1)
                acc = _Val(idx, acc.width + vb.width)
            vals[out0] = acc
            continue
        if op == "Concat":
            if int(a.get("axis", 0)) not in (1, -1) or any(i in inits for i in ins) or len(ins) < 2:
                raise PlanError("Concat is lowered along the feature axis of two or more branches")
            acc = plain(ins[0], op)
            for nxt in ins[1:]:
                vb = plain(nxt, op)
                if acc.width <= 0 or vb.width <= 0:
                    raise PlanError("Concat: branch widths must be known")
                idx = emit(JoinStep("concat", acc.step, vb.step, acc.width, vb.width), -1)
                acc = _Val(idx, acc.width + vb.width)
            vals[n["outputs"][0]] = acc
            continue
        if op == "Clip":
            lo, hi = -np.inf, np.inf
            for k, key in ((1, "min"), (2, "max")):
                if len(ins) > k and ins[k]:
                    if ins[k] not in inits:
                        raise PlanError(f"Clip: {key} must be a constant (an attribute or an initializer)")
                    c = float(np.asarray(const(ins[k]), np.float64).ravel()[0])
                    lo, hi = (c, hi) if k == 1 else (lo, c)
            lo, hi = float(a.get("min", lo)), float(a.get("max", hi))
            if lo == 0.0 and hi == np.inf:
                op = "Relu"   # clamp(min=0): folds like a Relu below
            else:
                f32 = float(np.finfo(np.float32).max)
                row_act(x, n["outputs"][0], op, "clip", max(lo, -f32), min(hi, f32))
                continue
        if op in ACT_OPS:
            v = plain(x, op)
            st = steps[v.step] if v.step >= 0 else None
            if (st is not None and st.kind in ("dense", "qdense") and st.act == "none"
                    and getattr(st, "out_q", None) is None and v.exclusive and single_use(x)):
                st.act = op.lower()
            elif (st is not None and st.kind == "tree" and op == "Sigmoid" and st.post == 0 and st.binary_class < 0
                  and v.exclusive and single_use(x)):
                st.post = 1
            elif (st is not None and st.kind == "svm" and op == "Sigmoid" and st.act == "none"
                  and v.exclusive and single_use(x)):
                st.act = "sigmoid"
            else:   # after a join, a tree, another activation, or on a value with other readers
                row_act(x, n["outputs"][0], op, op.lower())
                continue
            vals[n["outputs"][0]] = replace(v)
            continue
        if op in ROW_ACT_OPS:
            act, k0, k1 = ROW_ACT_OPS[op]
            if op == "Gelu":
                approx = str(a.get("approximate", "none"))
                if approx not in ("none", "tanh"):
                    raise PlanError(f"Gelu: approximate {approx!r} is not lowered")
                act = "gelu_tanh" if approx == "tanh" else "gelu"
            row_act(x, n["outputs"][0], op, act, float(a.get(*k0)) if k0 else 0.0, float(a.get(*k1)) if k1 else 0.0)
            continue
        if op == "PRelu":
            if len(ins) < 2 or ins[1] not in inits:
                raise PlanError("PRelu: the slope must be a constant (an initializer)")
            slope = np.asarray(const(ins[1]), np.float32).ravel()
            w = get(x, op).width
            if slope.size == 1:
                row_act(x, n["outputs"][0], op, "prelu", float(slope[0]))
            elif slope.size == w:
                row_act(x, n["outputs"][0], op, "prelu", gamma=slope)
            else:
                raise PlanError(f"PRelu: {slope.size} slopes for width {w} (one, or one per column)")
            continue
        if op == "BatchNormalization":
            if int(a.get("training_mode", 0)):
                raise PlanError("BatchNormalization: training_mode=1 is not lowered (inference only)")
            if len(ins) < 5 or any(i not in inits for i in ins[1:5]):
                raise PlanError("BatchNormalization: scale, B, mean and var must be initializers")
            if any(o and o in reads for o in n["outputs"][1:]):
                raise PlanError("BatchNormalization: the running statistics outputs are not lowered")
            g_, b_, mu, var = (np.asarray(const(i), np.float64).ravel() for i in ins[1:5])
            sc = g_ / np.sqrt(var + float(a.get("epsilon", 1e-5)))
            affine(x, n["outputs"][0], op, scale=sc, shift=b_ - mu * sc)
            continue
        if op == "LayerNormalization":
            if int(a.get("axis", -1)) not in (-1, 1):
                raise PlanError(f"LayerNormalization: axis {int(a.get('axis', -1))} is not lowered (last axis only)")
            if any(o and o in reads for o in n["outputs"][1:]):
                raise PlanError("LayerNormalization: the Mean / InvStdDev outputs are not lowered")
            if len(ins) < 2 or ins[1] not in inits or (len(ins) > 2 and ins[2] and ins[2] not in inits):
                raise PlanError("LayerNormalization: Scale (required) and B must be initializers")
            v = plain(x, op)
            gam = np.asarray(const(ins[1]), np.float32).ravel()
            bet = np.asarray(const(ins[2]), np.float32).ravel() if len(ins) > 2 and ins[2] else None
            if v.width <= 0 or gam.size != v.width or (bet is not None and bet.size != v.width):
                raise PlanError(f"LayerNormalization: Scale / B do not match the width {v.width}")
            idx = emit(RowStep("layernorm", v.width, eps=float(a.get("epsilon", 1e-5)), gamma_np=gam, beta_np=bet),
                       v.step)
            vals[n["outputs"][0]] = _Val(idx, v.width)
            continue
        if op == "Softmax":
            if int(a.get("axis", -1)) not in (-1, 1):
                raise PlanError(f"Softmax: axis {int(a.get('axis', -1))} is not lowered (the feature axis only)")
            v = plain(x, op)
            st = steps[v.step] if v.step >= 0 else None
            if (st is not None and st.kind == "dense" and st.act == "none" and st.n == 2 and v.exclusive
                    and single_use(x)):
                # softmax over two logits: p1 = sigmoid(z1 - z0), one column (as LinearClassifier SOFTMAX)
                w64 = st.w_np.astype(np.float64)
                b64 = np.zeros(2) if st.b_np is None else st.b_np.astype(np.float64)
                st.w_np = np.ascontiguousarray(w64[1:] - w64[:1], np.float32)
                st.b_np = (b64[1:] - b64[:1]).astype(np.float32)
                st.n, st.act = 1, "sigmoid"
                vals[n["outputs"][0]] = _Val(v.step, 1, ml_col=0, cpu_col=1, narrowed=True)
                continue
            if v.width <= 0:
                raise PlanError("Softmax: the width of its input must be known")
            idx = emit(RowStep("softmax", v.width), v.step)
            col = 1 if v.width == 2 else 0
            vals[n["outputs"][0]] = _Val(idx, v.width, ml_col=col, cpu_col=col)
            continue
        if op in ALIAS_OPS:
            if x not in vals:
                raise PlanError(f"{op}: value {x!r} is not computed by a lowered node")
            v = vals[x]
            if op == "Dropout":
                if len(n["outputs"]) > 1 and n["outputs"][1] and n["outputs"][1] in reads:
                    raise PlanError("Dropout: its mask output is read, which is not lowered")
                if len(ins) > 2 and ins[2] in inits and np.asarray(const(ins[2])).ravel()[:1].any():
                    raise PlanError("Dropout: training_mode is a constant true (inference only)")
            if op == "Reshape" and v.bidir_pending:
                raise PlanError(f"bidirectional {steps[v.step].kind.upper()}: Y_h [2, N, H] must be transposed to "
                                "[N, 2, H] before reshaping")
            if op == "Cast" and int(a.get("to", 1)) != 1:
                # to int32 / int64 as the sole link between a column view and a OneHotEncoder: the
                # encoder truncates the same way (NaN and out-of-range values match no category)
                readers = [m for m in order if out0 in m["inputs"]]
                if (int(a["to"]) not in (6, 7) or not readers or out0 in outs
                        or any(m["op_type"] != "OneHotEncoder" for m in readers)):
                    raise PlanError("Cast to a non-float type is not lowered")
                v = replace(view(x, op, rank1_ok=True), int_cast=True)
            elif op == "Cast" and v.int_cast:
                raise PlanError("Cast to a non-float type is not lowered")
            if v.cols is not None and v.onehot3d:
                # [N, C, n_cats] -> [N, C * n_cats]: column-major then category, the records' order
                shape = None
                if op == "Reshape" and len(ins) > 1 and ins[1] in raw_inits:
                    shape = [int(d) for d in np.asarray(model.initializer(ins[1])).ravel()]
                if (op == "Flatten" and int(a.get("axis", 1)) == 1) or (
                        shape is not None and len(shape) == 2 and shape[1] in (-1, v.width)
                        and shape[0] in (0, -1) and shape != [-1, -1]):
                    v = replace(v, onehot3d=False)
                elif op not in ("Identity", "Dropout", "Cast"):
                    raise PlanError(f"{op}: a OneHotEncoder output [N, C, n_cats] must be flattened to "
                                    "[N, C * n_cats] (Flatten axis 1 / Reshape) before anything else reads it")
            elif v.cols is not None and v.rank1 and op in ("Unsqueeze", "Reshape", "Flatten"):
                v = replace(v, rank1=False)   # [N] -> [N, 1]
            elif v.pool3d and op in ("Flatten", "Squeeze", "Reshape"):
                v = replace(v, pool3d=False)  # [N, C, 1] -> [N, C]
            vals[n["outputs"][0]] = v
            continue
        if op == "Transpose":
            # only the direction <-> batch swap of a layout-0 GRU's Y_h ([D, N, H] -> [N, D, H])
            v = vals.get(x)
            perm = [int(p) for p in a.get("perm", [])]
            if (v is None or v.step < 0 or not is_sequence_step(steps[v.step]) or steps[v.step].layout != 0
                    or perm != [1, 0, 2]):
                raise PlanError("Transpose is lowered only as perm [1, 0, 2] on a GRU's final states")
            vals[n["outputs"][0]] = replace(v, bidir_pending=False)
            continue
        if op == "GRU":
            v = vals.get(x)
            if v is None or v.scale is not None or (v.step >= 0 and not v.gru_y):
                raise PlanError("GRU: the input must be the model input or the previous layer's Y")
            direction = a.get("direction", "forward")
            layout = int(a.get("layout", 0))
            if direction not in ("forward", "reverse", "bidirectional") or layout not in (0, 1):
                raise PlanError(f"GRU: direction {direction!r} / layout {layout} is not lowered")
            masked = seq_lens("GRU", ins)
            if len(ins) > 5 and ins[5]:
                raise PlanError("GRU: initial_h is not lowered (the device starts every sequence at zero)")
            if any(s.kind == "lstm" for s in steps):
                raise PlanError("GRU: GRU and LSTM layers mixed in one chain are not lowered")
            prev = [s for s in steps if s.kind == "gru"]
            if prev and (direction == "bidirectional" or prev[0].bidirectional
                         or prev[0].reverse != (direction == "reverse") or prev[0].layout != layout):
                raise PlanError("GRU: stacked layers must share direction and layout (bidirectional: one layer)")
            Wa = np.asarray(const(ins[1]), np.float32)
            Ra = np.asarray(const(ins[2]), np.float32)
            H = int(a.get("hidden_size", Ra.shape[-1]))
            D = 2 if direction == "bidirectional" else 1
            Ba = (np.asarray(const(ins[3]), np.float32).reshape(D, 6 * H)
                  if len(ins) > 3 and ins[3] else np.zeros((D, 6 * H), np.float32))
            if Wa.shape[0] != D or Ra.shape[0] != D:
                raise PlanError("GRU: weight direction count does not match the direction attribute")
            seq = dims[1] if layout == 1 else dims[0]
            idx = emit(GRUStep(hidden=H, in_dim=int(Wa.shape[2]),
                               linear_before_reset=int(a.get("linear_before_reset", 0)),
                               w_np=Wa[0], r_np=Ra[0], b_np=Ba[0], seq=int(seq) if seq > 0 else 0,
                               reverse=direction == "reverse", layout=layout, bidirectional=D == 2,
                               w_rev_np=Wa[1] if D == 2 else None, r_rev_np=Ra[1] if D == 2 else None,
                               b_rev_np=Ba[1] if D == 2 else None, masked=masked), v.step)
            y, yh = n["outputs"][0], (n["outputs"][1] if len(n["outputs"]) > 1 else "")
            if D == 2 and y and uses.get(y, 0) > 0:
                raise PlanError("bidirectional GRU: only the final states (Y_h) are lowered")
            if y:
                vals[y] = _Val(idx, H * D, gru_y=True)
            if yh:
                vals[yh] = _Val(idx, H * D, bidir_pending=D == 2 and layout == 0)
            continue
        if op == "LSTM":
            v = vals.get(x)
            if v is None or v.scale is not None or (v.step >= 0 and not v.gru_y):
                raise PlanError("LSTM: the input must be the model input or the previous layer's Y")
            direction = a.get("direction", "forward")
            layout = int(a.get("layout", 0))
            if direction not in ("forward", "reverse", "bidirectional") or layout not in (0, 1):
                raise PlanError(f"LSTM: direction {direction!r} / layout {layout} is not lowered")
            D = 2 if direction == "bidirectional" else 1
            masked = seq_lens("LSTM", ins)
            if len(ins) > 5 and ins[5]:
                raise PlanError("LSTM: initial_h is not lowered (the device starts every sequence at zero)")
            if len(ins) > 6 and ins[6]:
                raise PlanError("LSTM: initial_c is not lowered (the device starts every cell state at zero)")
            if len(ins) > 7 and ins[7]:
                raise PlanError("LSTM: peepholes (P) are not lowered")
            acts = [str(s) for s in a.get("activations", [])]
            if acts and acts != ["Sigmoid", "Tanh", "Tanh"] * D:
                raise PlanError(f"LSTM: activations {acts} are not lowered (Sigmoid / Tanh / Tanh only)")
            if "activation_alpha" in a or "activation_beta" in a:
                raise PlanError("LSTM: activations with alpha / beta are not lowered")
            if "clip" in a:
                raise PlanError("LSTM: clip is not lowered")
            if int(a.get("input_forget", 0)):
                raise PlanError("LSTM: input_forget = 1 is not lowered")
            if any(s.kind == "gru" for s in steps):
                raise PlanError("LSTM: GRU and LSTM layers mixed in one chain are not lowered")
            prev = [s for s in steps if s.kind == "lstm"]
            if prev and (D == 2 or prev[0].bidirectional
                         or prev[0].reverse != (direction == "reverse") or prev[0].layout != layout):
                raise PlanError("LSTM: stacked layers must share direction and layout (bidirectional: one layer)")
            Wa = np.asarray(const(ins[1]), np.float32)
            Ra = np.asarray(const(ins[2]), np.float32)
            H = int(a.get("hidden_size", Ra.shape[-1]))
            Ba = (np.asarray(const(ins[3]), np.float32).reshape(D, 8 * H)
                  if len(ins) > 3 and ins[3] else np.zeros((D, 8 * H), np.float32))
            if Wa.shape[0] != D or Ra.shape[0] != D:
                raise PlanError("LSTM: weight direction count does not match the direction attribute")
            if Wa.shape[1] != 4 * H or Ra.shape[1:] != (4 * H, H):
                raise PlanError("LSTM: W / R must be [D, 4H, I] / [D, 4H, H]")
            outs_n = list(n["outputs"]) + ["", "", ""]
            y, yh, yc = outs_n[0], outs_n[1], outs_n[2]
            if yc and (uses.get(yc, 0) > 0 or yc in outs):
                raise PlanError("LSTM: the final cell state Y_c is consumed, which is not lowered")
            seq = dims[1] if layout == 1 else dims[0]
            idx = emit(LSTMStep(hidden=H, in_dim=int(Wa.shape[2]), w_np=Wa[0], r_np=Ra[0], b_np=Ba[0],
                                seq=int(seq) if seq > 0 else 0, reverse=direction == "reverse", layout=layout,
                                bidirectional=D == 2, w_rev_np=Wa[1] if D == 2 else None,
                                r_rev_np=Ra[1] if D == 2 else None, b_rev_np=Ba[1] if D == 2 else None,
                                masked=masked), v.step)
            if D == 2 and y and uses.get(y, 0) > 0:
                raise PlanError("bidirectional LSTM: only the final states (Y_h) are lowered")
            if y:
                vals[y] = _Val(idx, H * D, gru_y=True)
            if yh:
                vals[yh] = _Val(idx, H * D, bidir_pending=D == 2 and layout == 0)
            continue
        if op in ("LinearClassifier", "LinearRegressor"):
            coef = np.asarray(a.get("coefficients", []), np.float64).ravel()
            icpt = np.asarray(a.get("intercepts", []), np.float64).ravel()
            post = str(a.get("post_transform", "NONE"))
            if op == "LinearRegressor":
                E = int(a.get("targets", 1))
            else:
                E = len(icpt) if len(icpt) else max(1, coef.size // max(vals[x].width, 1) if x in vals else 1)
            if E < 1 or coef.size % E:
                raise PlanError(f"{op}: coefficients do not split into {E} rows")
            w = coef.reshape(E, coef.size // E).T           # [C, E]
            b = icpt if len(icpt) else np.zeros(E)
            if len(b) != E:
                raise PlanError(f"{op}: {len(b)} intercepts for {E} rows")
            col = cpu = 0
            narrowed = False
            if op == "LinearClassifier" and E == 2 and post == "SOFTMAX":
                # softmax over two scores: p1 = sigmoid(s1 - s0), one column
                w, b, act = w[:, 1:] - w[:, :1], b[1:] - b[:1], "sigmoid"
                narrowed, cpu = True, 1
            elif op == "LinearClassifier" and E == 1 and post == "SOFTMAX":
                # one row: softmax over [-s, s] -> p1 = sigmoid(2 s)
                w, b, act = 2 * w, 2 * b, "sigmoid"
                narrowed, cpu = True, 1
            elif post in LINEAR_POST:
                act = LINEAR_POST[post]
                if op == "LinearClassifier" and E == 1:
                    narrowed, cpu = True, 1   # executor scores [-s, s] (LOGISTIC: sigmoid of both)
                elif op == "LinearClassifier" and E == 2:
                    col = cpu = 1
            else:
                raise PlanError(f"{op}: post_transform {post} with {E} rows is CPU-only")
            src, w32, b32 = linear(x, w.astype(np.float32), b.astype(np.float32), op)
            idx = emit(DenseStep(n=int(w32.shape[1]), k=int(w32.shape[0]), act=act,
                                 w_np=np.ascontiguousarray(w32.T, np.float32), b_np=b32), src)
            scores = _Val(idx, int(w32.shape[1]), ml_col=col, cpu_col=cpu, narrowed=narrowed)
            if op == "LinearClassifier":
                vals[n["outputs"][0]] = _Val(idx, 1, label=True)
                if len(n["outputs"]) > 1:
                    vals[n["outputs"][1]] = scores
            else:
                vals[n["outputs"][0]] = scores
            continue
        if op == "Neg":
            affine(x, n["outputs"][0], op, scale=-1.0)
            continue
        if op in ("SVMClassifier", "SVMRegressor"):
            info = ex.svm_info(index[id(n)])
            v = get(x, op)   # a pending Scaler / constant affine becomes the step's input stage
            F_, S_ = int(info["n_feat"]), int(info["n_sv"])
            if v.width > 0 and v.width != F_:
                raise PlanError(f"{op}: support vectors have {F_} columns, the input {v.width}")
            if F_ > SVM_MAX_F:
                raise PlanError(f"{op}: {F_} input columns (> {SVM_MAX_F}) are CPU-only")
            kern = SVM_KERNELS[int(info["kernel"])]
            deg = float(info["degree"])
            if kern == "POLY" and (deg != int(deg) or not 0 <= deg <= SVM_MAX_DEGREE):
                raise PlanError(f"{op}: POLY degree {deg:g} is CPU-only (the device takes integers in [0, {SVM_MAX_DEGREE}])")
            post = POST[int(info["post"])]
            if post not in LINEAR_POST:
                raise PlanError(f"{op}: post_transform {post} is CPU-only")
            for what_, t in (("scale", v.scale), ("shift", v.shift)):
                if t is not None and len(t) not in (1, F_):
                    raise PlanError(f"{op}: {len(t)} per-column input constants for {F_} columns")
            ss = SVMStep(kernel=kern, gamma=float(info["gamma"]), coef0=float(info["coef0"]),
                         degree=int(deg) if kern == "POLY" else 0, n_sv=S_, in_dim=F_,
                         sv_np=np.ascontiguousarray(info["sv"], np.float32),
                         coef_np=np.ascontiguousarray(info["coef"], np.float32), rho=float(info["rho"]),
                         in_scale=None if v.scale is None else np.array(np.broadcast_to(v.scale, (F_,)), np.float64),
                         in_shift=None if v.shift is None else np.array(np.broadcast_to(v.shift, (F_,)), np.float64))
            if info["classifier"]:
                # the positive column (classlabels[1]): 1 - p0 with Platt, else post(-dec)
                if info["platt"]:
                    ss.platt, ss.platt_flip = (float(info["prob_a"]), float(info["prob_b"])), True
                else:
                    ss.post_scale, ss.act = -1.0, LINEAR_POST[post]
                idx = emit(ss, v.step)
                vals[n["outputs"][0]] = _Val(idx, 1, label=True)
                if len(n["outputs"]) > 1 and n["outputs"][1]:
                    vals[n["outputs"][1]] = _Val(idx, 1, ml_col=0, cpu_col=1, narrowed=True)
            else:
                ss.one_class, ss.act = bool(info["one_class"]), LINEAR_POST[post]
                idx = emit(ss, v.step)
                vals[n["outputs"][0]] = _Val(idx, 1)
            continue
        if op == "Scaler":
            off = np.asarray(a.get("offset", [0.0]), np.float64).ravel()
            sc = np.asarray(a.get("scale", [1.0]), np.float64).ravel()
            if len(off) > 1 and len(sc) == 1:
                sc = np.full(len(off), sc[0])
            if len(sc) > 1 and len(off) == 1:
                off = np.full(len(sc), off[0])
            affine(x, n["outputs"][0], op, scale=sc, shift=-off * sc)
            continue
        raise PlanError(f"op {op} is not lowered to the device")

    if output_name in seqs:
        raise PlanError("the output is a sequence value [N, C, T]: a read-out (last step, mean, max or sum over time) "
                        "must follow")
    fv = vals.get(output_name)
    if fv is None or fv.label or fv.quant is not None or fv.pool3d:
        raise PlanError("the primary output must be a score / probability tensor")
    if fv.deq is not None or fv.cols is not None:
        # a trailing Q -> DQ: the DequantizeLinear is the last step; a column view: its ColumnStep
        fv = get(output_name, "output")
    if fv.scale is not None:
        fv = plain(output_name, "output")
    if not steps or fv.step != len(steps) - 1:
        raise PlanError("the output must be computed by the last lowered step")
    if has_sequence(steps) and any(s.kind == "row" for s in steps):
        s = next(s for s in steps if s.kind == "row")
        raise PlanError(f"sequence models are lowered as chains (GRU / LSTM layers + head) only: a row step "
                        f"({s.act if s.op == 'act' else s.op}) in a sequence plan is not lowered")
    convs = any(s.kind == "conv" for s in steps)
    if not convs and has_sequence(steps) and any(s.kind == "join" or s.src != i - 1 for i, s in enumerate(steps)):
        raise PlanError("sequence models are lowered as chains (GRU / LSTM layers + head) only")
    if convs:
        kinds = [s.kind for s in steps]
        p = kinds.index("seqpool") if "seqpool" in kinds else len(kinds)
        if kinds.count("seqpool") != 1 or any(k != "conv" for k in kinds[:p]):
            raise PlanError("a temporal-convolution model is lowered as convolution layers and one read-out")
        for i, s in enumerate(steps[p + 1:], p + 1):
            if s.kind != "dense" or s.src != i - 1:
                raise PlanError(f"sequence models are lowered as convolution layers, a read-out and a chain of dense layers "
                                f"only: a {s.kind} step behind the read-out is not lowered")
        for s in steps[:p]:
            check_conv(s)
    fam = model.metadata.get("family", "")
    if not fam:
        kinds = [s.kind for s in steps if s.kind != "cols"]   # a column front end keeps the estimator's family
        fam = ("svm" if kinds == ["svm"] else "gbdt" if kinds == ["tree"] else "stacked" if kinds and kinds[0] == "tree"
               else "gru" if "gru" in kinds else "lstm" if "lstm" in kinds else "tcn" if "conv" in kinds else "mlp")
    plan = Plan(family=fam, in_width=in_width, steps=steps, out_width=fv.width, ml_col=fv.ml_col,
                metadata=dict(model.metadata), input_name=input_name, output_name=output_name,
                seq_input=seq_input, cpu_col=fv.cpu_col, lens_input=lens_seen[0] if lens_seen else None)
    # (a TCN's trailing dense layers stay dense steps: runner.TcnModel runs them one by one)
    return fuse(plan) if fuse_heads and not convs else fuse(plan, heads=False)


def sequence_lens_input(model) -> Optional[str]:
    """The graph input a model's GRU / LSTM nodes read as ONNX sequence_lens (None: unmasked). No
    lowering: the CPU executor paths ask this of models the device may not run."""
    inputs = {v[0] for v in model.inputs()} - set(model.initializer_names())
    for n in model.nodes():
        if n["op_type"] in ("GRU", "LSTM") and len(n["inputs"]) > 4 and n["inputs"][4] in inputs:
            return n["inputs"][4]
    return None


def executor_output(model, default_output: str = "output") -> Tuple[int, str]:
    """(score column, output name) of the model's primary output in the C++ CPU executor -
    also for models the device cannot run (the plan's view when it compiles; otherwise the
    last graph output, column 1 for a two-class classifier's probabilities)."""
    try:
        p = compile_onnx(model, output_name=default_output)
        return p.executor_col, p.output_name
    except Exception:  # PlanError, or a graph the lowering cannot even walk: the executor still runs it
        pass
    outs = [v[0] for v in model.outputs()]
    name = default_output if default_output in outs else outs[-1]
    nodes = model.nodes()
    prod = {o: n for n in nodes for o in n["outputs"] if o}
    n = prod.get(name)
    while n is not None and n["op_type"] in ALIAS_OPS:
        n = prod.get(n["inputs"][0])
    col = 0
    if n is not None and n["op_type"] == "LinearClassifier":
        icpt = np.asarray(n["attrs"].get("intercepts", []))
        col = 1 if len(icpt) in (1, 2) else 0
    elif n is not None and n["op_type"] == "SVMClassifier":
        col = 1
    elif n is not None and n["op_type"] == "TreeEnsembleClassifier":
        col = 1 if len(np.asarray(n["attrs"].get("classlabels_int64s", n["attrs"].get("classlabels_strings", [])))) == 2 else 0
    return col, name


def fuse(plan: Plan, heads: bool = True) -> Plan:
    """Fusion pass: dense(N>1) followed by dense(N=1) that alone reads it -> HeadStep (no
    hidden tensor in HBM). Step inputs are then renumbered and stored implicitly (``src`` None)
    wherever a step reads its predecessor."""
    st = plan.steps
    ins = [step_inputs(st, i) for i in range(len(st))]
    cons = step_consumers(st)
    out, origin, remap = [], [], {-1: -1}
    i = 0
    while i < len(st):
        s = st[i]
        if (heads and s.kind == "dense" and s.n > 1 and i + 1 < len(st) and st[i + 1].kind == "dense"
                and st[i + 1].n == 1 and ins[i + 1] == (i,) and cons[i] == [i + 1]
                and s.n <= 4096 and s.k <= 1024):
            t = st[i + 1]
            out.append(HeadStep(n1=s.n, k=s.k, act1=s.act, act2=t.act, w1_np=s.w_np, b1_np=s.b_np,
                                w2_np=np.ascontiguousarray(t.w_np[0], np.float32),
                                b2=float(t.b_np[0]) if t.b_np is not None else 0.0))
            origin.append(i)
            remap[i] = remap[i + 1] = len(out) - 1
            i += 2
            continue
        out.append(s)
        origin.append(i)
        remap[i] = len(out) - 1
        i += 1
    for j, (s, oi) in enumerate(zip(out, origin)):
        if s.kind == "join":
            s.a, s.b = remap[s.a], remap[s.b]
        else:
            src = remap[ins[oi][0]]
            s.src = None if src == j - 1 else src
            if s.kind == "conv" and s.res is not None:
                s.res = remap[s.res]
    plan.steps = out
    return plan


def _bf16_padded(w: np.ndarray, n_mult: int = 128, k_mult: int = 64):
    import torch
    n, k = w.shape
    npad = -(-n // n_mult) * n_mult
    kpad = -(-k // k_mult) * k_mult
    buf = np.zeros((npad, kpad), np.float32)
    buf[:n, :k] = w
    return torch.from_numpy(buf).to(torch.bfloat16)


def _f32_padded(w: np.ndarray, n_mult: int = 128, k_mult: int = 64):
    import torch
    n, k = w.shape
    buf = np.zeros((-(-n // n_mult) * n_mult, -(-k // k_mult) * k_mult), np.float32)
    buf[:n, :k] = w
    return torch.from_numpy(buf)


PRECISIONS = ("fp32", "bf16")

SET_CAP = 256            # csrc/runtime/trees.h SET_CAP: bitsets hold the integers [0, SET_CAP)
SET_LIST = 0x80000000    # set header: kind << 31 | length


def validate_sets(sets: Optional[np.ndarray], offsets: np.ndarray, what: str) -> None:
    """Host check of the member-set table against the offsets its BRANCH_MEMBER nodes carry:
    every header and every set body lies inside the table, a bitset has at most SET_CAP / 32
    words, a value list is strictly increasing and holds no NaN. The device test then reads
    inside the table only."""
    tab = np.zeros(0, np.uint32) if sets is None else np.asarray(sets)
    if tab.dtype != np.uint32 or tab.ndim != 1:
        raise PlanError(f"{what}: the set table must be a flat uint32 array")
    W = int(tab.size)
    for off in np.unique(np.asarray(offsets).astype(np.int64)):
        off = int(off)
        if off < 0 or off >= W:
            raise PlanError(f"{what}: set offset {off} outside the table of {W} words")
        h = int(tab[off])
        n = h & ~SET_LIST
        if off + 1 + n > W:
            raise PlanError(f"{what}: set at {off} has length {n}, past the table of {W} words")
        if not h & SET_LIST:
            if n * 32 > SET_CAP:
                raise PlanError(f"{what}: bitset at {off} has {n} words (> {SET_CAP // 32})")
            continue
        v = tab[off + 1:off + 1 + n].view(np.float32)
        if np.isnan(v).any():
            raise PlanError(f"{what}: value list at {off} contains NaN")
        if n > 1 and not (v[1:] > v[:-1]).all():
            raise PlanError(f"{what}: value list at {off} is not sorted and distinct")


def validate_complete(s: TreeStep) -> None:
    """Host check of a complete-layout ensemble's member nodes (the layout itself is implicit)."""
    nd = s.nodes_np.reshape(-1, 2).view(np.uint32)
    member = ((nd[:, 1] >> 16) & 7) == 6
    if member.any() or (s.sets_np is not None and s.sets_np.size):
        validate_sets(s.sets_np, nd[member, 0], "complete trees")


def validate_sparse(s: TreeStep) -> None:
    """Host check of a pointer-layout ensemble before it reaches the device: every child / root
    index is a node, every leaf row exists, and no root-to-leaf path is longer than ``depth``
    (the kernel's traversal bound), so K2b can only read inside its arrays."""
    nodes = s.nodes_np.reshape(-1, 4)
    N, L = nodes.shape[0], s.leaf_w_np.shape[0]
    if s.leaf_w_np.shape != (L, s.k) or s.leaf_has_np.shape != (L, s.k):
        raise PlanError("sparse trees: leaf tables must be [L, K]")
    if s.roots_np.shape != (s.n_trees,) or (s.roots_np < 0).any() or (s.roots_np >= N).any():
        raise PlanError("sparse trees: root index out of range")
    mode = (nodes[:, 0].view(np.uint32) >> 16) & 7
    leaf = mode == 7
    if ((nodes[leaf, 2] < 0) | (nodes[leaf, 2] >= L)).any():
        raise PlanError("sparse trees: leaf row out of range")
    ch = nodes[~leaf][:, 2:4]
    if ((ch < 0) | (ch >= N)).any():
        raise PlanError("sparse trees: child index out of range")
    member = mode == 6
    if member.any() or (s.sets_np is not None and s.sets_np.size):
        validate_sets(s.sets_np, nodes[member, 1].view(np.uint32), "sparse trees")
    # initial -1: an ensemble of single-leaf trees reads no feature (max_feature = -1)
    if (nodes[~leaf, 0].view(np.uint32) & 0xFFFF).astype(np.int64).max(initial=-1) > s.max_feature:
        raise PlanError("sparse trees: feature id above max_feature")
    # longest path by level expansion from the roots (bounded by depth + 1 levels)
    frontier = s.roots_np.astype(np.int64)
    for _ in range(s.depth + 1):
        inner = frontier[~leaf[frontier]]
        if inner.size == 0:
            return
        frontier = np.unique(np.concatenate([nodes[inner, 2], nodes[inner, 3]]).astype(np.int64))
    raise PlanError("sparse trees: a path is longer than the declared depth (cycle?)")


def to_device(plan: Plan, device, precision: str = "fp32") -> Plan:
    """Upload the plan's tensors. ``precision`` selects the dense / head weight format:
    ``fp32`` (default) keeps the ONNX model's f32 numerics end to end (f32 MFMA,
    onnx_model.go:221-238 contract); ``bf16`` runs the dense layers on the bf16 MFMA path
    (f32 accumulate). Trees are always f32; GRU weights are always bf16 (K4)."""
    import torch
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    plan.precision = precision
    pad = _f32_padded if precision == "fp32" else _bf16_padded
    for s in plan.steps:
        if s.kind == "tree":
            (validate_sparse if s.layout == "sparse" else validate_complete)(s)  # before any upload
            s.nodes = torch.from_numpy(s.nodes_np).to(device)
            s.base = None if s.base_np is None else torch.from_numpy(s.base_np).to(device)
            s.sets = (None if s.sets_np is None or s.sets_np.size == 0
                      else torch.from_numpy(np.ascontiguousarray(s.sets_np, np.uint32).view(np.int32)).to(device))
            if s.layout == "sparse":
                s.roots = torch.from_numpy(s.roots_np).to(device)
                s.leaf_w = torch.from_numpy(s.leaf_w_np).to(device)
                s.leaf_has = torch.from_numpy(s.leaf_has_np).to(device)
            else:
                s.leaves = torch.from_numpy(s.leaves_np).to(device)
        elif s.kind == "dense":
            s.w = pad(s.w_np).to(device)
            s.b = None if s.b_np is None else torch.from_numpy(np.ascontiguousarray(s.b_np)).to(device)
        elif s.kind == "head":
            # f32 head: K padded to 32 only (the f32 MFMA k-step is 16; the specialised kernel is
            # built for k_pad 32 / 64), so a 32-wide tree embedding runs no all-zero k-steps
            s.w1 = (_f32_padded(s.w1_np, k_mult=32) if precision == "fp32" else pad(s.w1_np)).to(device)
            s.b1 = None if s.b1_np is None else torch.from_numpy(np.ascontiguousarray(s.b1_np)).to(device)
            s.w2 = torch.from_numpy(s.w2_np).to(device)
        elif s.kind == "svm":
            validate_svm(s)   # before any upload
            t = svm_tables(s)
            s.sv, s.coef, s.scale, s.shift = (t[k].to(device) for k in ("sv", "coef", "scale", "shift"))
            s.sv_norm = None if t["sv_norm"] is None else t["sv_norm"].to(device)
        elif s.kind == "cols":
            upload_columns(s, device)   # the host check, then the table
        elif s.kind == "conv":
            check_conv(s)   # before any upload
            t = conv_tables(s)
            s.w, s.b = t["w"].to(device), t["bias"].to(device)
        elif s.kind == "qdense":
            t = qdense_tables(s)
            s.w8, s.corr, s.mult, s.b = (t[k].to(device) for k in ("w8", "corr", "mult", "bias"))
        elif s.kind == "row":
            s.gamma, s.beta = (None if t is None else torch.from_numpy(np.ascontiguousarray(t, np.float32)).to(device)
                               for t in (s.gamma_np, s.beta_np))
    return plan


def gru_device_weights(s: GRUStep, device) -> Dict[str, Any]:
    import torch
    H = s.hidden
    d = {
        "R": torch.from_numpy(np.ascontiguousarray(s.r_np)).to(torch.bfloat16).to(device),
        "bias": torch.from_numpy(np.ascontiguousarray(s.b_np, np.float32)).to(device),
        # input projection as a dense layer [3H, I] (W rows are output columns already)
        "W": _bf16_padded(np.ascontiguousarray(s.w_np)).to(device),
        "Wb": torch.from_numpy(np.ascontiguousarray(s.b_np[:3 * H], np.float32)).to(device),
    }
    return d
