"""Device execution of a compiled :class:`Plan` (tree / dense / fused head / GRU steps).

Owns the per-step activation buffers (sized for the largest bucket), the tree-partial slab
used by the tree->head fusion and the per-bucket tree group counts. Launches are eager on the
current stream; callers (the fraud scorer, the LTV and abuse services) capture them in
their own hipGraphs together with their copies, so a model step never re-captures.
"""
from __future__ import annotations

import os

from typing import Dict, List, Optional, Sequence

import torch

from ..models.plan import Plan, has_sequence, step_consumers, step_inputs, step_qtype
from ..ops import kernels as K


def tree_groups(step, bucket: int) -> int:
    """Split the trees of one ensemble into ``g`` groups so a small batch still fills the
    256 CUs, without shrinking a group below 8 trees: >= 384 workgroups (3 groups at 8192 rows).
    Round 5 moved the target from 512 to 256 workgroups (at 8192 rows 2 groups instead of 4
    left more of the chip to K1 / the dedup insert: engine_only 151 vs 139 M, profiles/r5/eng/
    groups). After round 6's LDS traversal rework and at serving depth 6, 3 groups measured best
    (same box, interleaved: 2 / 3 / 4 groups engine_only 149.4 / 151.0 / 147.5 M, serving
    120.1 / 127.1 / 127.0 M, profiles/r6/al; 3 pairs 2 vs 3 groups: serving 119.7 / 122.8 / 122.7
    vs 125.5 / 126.4 / 127.1 M, engine_only flat, profiles/r6/am); 1 group drops to 91 M."""
    forced = int(os.environ.get("IGP_TREE_GROUPS", "0"))  # same-box A/B override
    if forced > 0:
        return max(1, min(forced, step.n_trees))
    tiles = -(-bucket // 64)
    return max(1, min(max(1, step.n_trees // 8), -(-384 // tiles)))


class GruModel:
    """The GRU part of a plan on the device (K4, csrc/kernels/gru*.hip):

    * forward or reverse layers (1-2, stacked): one launch, the N=1 head fused in its epilogue;
    * one bidirectional layer: a forward and a reverse launch, each writing its final state
      into its half of a [rows, 2H] buffer (the ONNX Y_h in [N, 2, H] order), then the N=1
      head as a dense launch.

    Input: dense X f32 [T, rows, I] (the ONNX layout-0 order; layout-1 plans are fed the same,
    see :meth:`DeviceModel.run`) or the store's event rings for ``slots``.

    A plan whose layers read ONNX ``sequence_lens`` gives masked packs (``masked``): short rows hold
    their state outside their live steps. Dense input takes the lengths as ``lens`` (int32 [rows];
    None: every row is ``T`` steps long), ring input takes them from the accounts' event counts."""

    kind = "gru"     # the plan step kind, weight pack and launch of the cell (LstmModel overrides)
    pack = K.GruPack
    launch = staticmethod(K.gru)

    def __init__(self, steps, device, split: bool, bmax: int):
        n = 0
        while n < len(steps) and steps[n].kind == self.kind:
            n += 1
        head = steps[n] if n < len(steps) and steps[n].kind == "dense" and steps[n].n == 1 else None
        if n == 0 or n + (head is not None) != len(steps):
            raise ValueError(f"sequence model must be {self.kind.upper()} layers followed by at most an N=1 head")
        g = steps[0]
        self.H = g.hidden
        self.seq = g.seq
        self.bidirectional = g.bidirectional
        self.head = head
        if g.bidirectional:
            if n != 1:
                raise ValueError(f"bidirectional {self.kind.upper()}: one layer")
            self.packs = [self.pack([g.direction(0)], None, device, split=split),
                          self.pack([g.direction(1)], None, device, split=split, reverse=True)]
            self.yh = [torch.zeros((bmax, self.H), dtype=torch.float32, device=device) for _ in range(2)]
            self.cat = torch.zeros((bmax, 2 * self.H), dtype=torch.float32, device=device)
        else:
            self.packs = [self.pack(steps[:n], head, device, split=split, reverse=g.reverse)]

    @property
    def has_head(self) -> bool:
        return self.head is not None

    @property
    def shares_intermediates(self) -> bool:
        """Whether two ``run`` calls in flight at once would write the same device buffers (the
        direction buffers of a bidirectional layer): the abuse runners then keep every pipeline slot
        on one stream."""
        return self.bidirectional

    @property
    def masked(self) -> bool:
        return self.packs[0].masked

    @property
    def split(self) -> bool:
        """f32-faithful (bf16 hi/lo, three MFMAs per product) weights."""
        return self.packs[0].split

    def run(self, n_rows: int, T: int, out: torch.Tensor, X: Optional[torch.Tensor] = None, store=None,
            slots: Optional[torch.Tensor] = None, m_ptr: Optional[torch.Tensor] = None,
            lens: Optional[torch.Tensor] = None) -> None:
        """``out``: [rows] probabilities with a head, else [rows, H * directions] final states."""
        kw = dict(X=X, store=store, slots=slots, m_ptr=m_ptr)
        if lens is not None:
            kw["lens"] = lens
        if not self.bidirectional:
            gp = self.packs[0]
            if self.head is not None:
                self.launch(gp, n_rows, T, out=out, **kw)
            else:
                self.launch(gp, n_rows, T, yh=out, **kw)
            return
        for gp, yh in zip(self.packs, self.yh):
            self.launch(gp, n_rows, T, yh=yh, **kw)
        dst = self.cat if self.head is not None else out
        torch.cat([self.yh[0][:n_rows], self.yh[1][:n_rows]], dim=1, out=dst[:n_rows])
        if self.head is not None:
            h = self.head
            K.dense(self.cat, h.w, h.b, out, n_rows, 1, 2 * self.H, act=h.act, m_ptr=m_ptr)


class LstmModel(GruModel):
    """The LSTM part of a plan on the device (K4 LSTM, csrc/kernels/lstm.hip): the same launch
    structure and interface as :class:`GruModel`, on ``LstmPack`` / ``lstm``."""

    kind = "lstm"
    pack = K.LstmPack
    launch = staticmethod(K.lstm)


class _NoClusterPack:
    """What the abuse runners ask of a recurrent weight pack, for a model that has none: no
    weight-stationary cluster path to disable, no split tile to size."""
    ws_ok = wsx_ok = False
    x3_rows = 16    # ignored

    def disable_ws(self, keep_wsx: bool = False) -> None:
        pass


class TcnModel:
    """A temporal-convolution plan on the device (csrc/kernels/conv1d.hip): one ``conv1d`` launch per
    ConvStep, the ``seq_pool`` read-out, then the trailing dense layers (the N=1 head included) as
    ``dense`` launches. f32 convolutions whatever the plan's precision. The interface is
    :class:`GruModel`'s: dense X f32 [T, rows, I] or the store's event rings for ``slots`` (each
    account's last min(ev_count, T) events right-aligned, zeros before them).

    Activations are channel-last [rows, T, C_pad] f32 buffers: one per live value, shared between the
    steps whose outputs are never live together (two ping-pong buffers for a plain stack; a residual
    source keeps its buffer until its last reader has run)."""

    bidirectional = False
    split = False
    masked = False
    # one set of activation buffers: two runs in flight would overwrite each other's layers, so the
    # abuse runners keep their pipeline slots on one stream (as for a bidirectional GRU)
    shares_intermediates = True

    def __init__(self, steps, device, split: bool, bmax: int):
        kinds = [s.kind for s in steps]
        if "seqpool" not in kinds:
            raise ValueError("a temporal-convolution model needs a read-out (seqpool) step")
        p = kinds.index("seqpool")
        if p == 0 or any(k != "conv" for k in kinds[:p]):
            raise ValueError("a temporal-convolution model must be convolution layers followed by one read-out")
        if any(k != "dense" for k in kinds[p + 1:]):
            bad = next(k for k in kinds[p + 1:] if k != "dense")
            raise ValueError(f"a temporal-convolution model runs only dense layers behind its read-out, not {bad!r}")
        for i in range(p + 1, len(steps)):
            if step_inputs(steps, i) != (i - 1,):
                raise ValueError("the layers behind the read-out must form a chain")
        self.steps, self.n_conv, self.device = list(steps), p, device
        self.seq = steps[0].seq
        self.packs = [_NoClusterPack()]
        last = steps[-1]
        self.head = last if last.kind == "dense" and last.n == 1 else None
        # the last step reading each conv output; a buffer is free again after it
        last_read = {}
        for i in range(p + 1):
            for j in step_inputs(steps, i):
                last_read[j] = i
        T = max(int(self.seq), 1)
        self.bufs: List[torch.Tensor] = []
        self.buf_of: List[int] = []
        width = -(-max(s.c_out for s in steps[:p]) // 4) * 4
        holder: List[int] = []   # per buffer, the step whose output it holds
        for i in range(p):
            # a buffer is free once its value's last reader ran before this step (so never an input of step i)
            b = next((b for b, j in enumerate(holder) if last_read.get(j, -1) < i), None)
            if b is None:
                self.bufs.append(torch.zeros((bmax, T, width), dtype=torch.float32, device=device))
                holder.append(i)
                b = len(self.bufs) - 1
            holder[b] = i
            self.buf_of.append(b)
        self.T_alloc = T
        pool = steps[p]
        self.pooled = torch.zeros((bmax, pool.width), dtype=torch.float32, device=device)
        self.mid = [torch.zeros((bmax, s.n), dtype=torch.float32, device=device) for s in steps[p + 1:-1]]

    @property
    def has_head(self) -> bool:
        return self.head is not None

    def run(self, n_rows: int, T: int, out: torch.Tensor, X: Optional[torch.Tensor] = None, store=None,
            slots: Optional[torch.Tensor] = None, m_ptr: Optional[torch.Tensor] = None,
            lens: Optional[torch.Tensor] = None) -> None:
        """``out``: [rows] probabilities with an N=1 head, else [rows, width] of the last step."""
        if lens is not None:
            raise ValueError("a temporal-convolution model takes no sequence lengths")
        if T != self.T_alloc:
            raise ValueError(f"the model runs {self.T_alloc} time steps, not {T}")
        steps, p = self.steps, self.n_conv
        for i in range(p):
            s = steps[i]
            src = step_inputs(steps, i)[0]
            Y = self.bufs[self.buf_of[i]]
            res = None if s.res is None else self.bufs[self.buf_of[s.res]]
            if src < 0:
                K.conv1d(s, n_rows, T, Y, X=X, store=store, slots=slots, res=res, m_ptr=m_ptr)
            else:
                K.conv1d(s, n_rows, T, Y, A=self.bufs[self.buf_of[src]], res=res, m_ptr=m_ptr)
        pool = steps[p]
        tail = steps[p + 1:]
        out2 = out.view(-1, 1) if out.dim() == 1 else out
        src_buf = self.bufs[self.buf_of[step_inputs(steps, p)[0]]]
        K.seq_pool(pool.op, src_buf, self.pooled if tail else out2, n_rows, T, pool.width, m_ptr=m_ptr)
        cur = self.pooled
        for j, s in enumerate(tail):
            dst = out2 if j == len(tail) - 1 else self.mid[j]
            K.dense(cur, s.w, s.b, dst, n_rows, s.n, s.k, act=s.act, m_ptr=m_ptr)
            cur = dst


def sequence_model(steps, device, split: bool, bmax: int):
    """The device runner of a sequence plan: GRU or LSTM layers (+ head), or a temporal-convolution
    network (convolution layers, read-out, dense layers)."""
    if steps and steps[0].kind == "conv":
        return TcnModel(steps, device, split, bmax)
    if steps and steps[0].kind == "lstm":
        return LstmModel(steps, device, split, bmax)
    return GruModel(steps, device, split, bmax)


class DeviceModel:
    def __init__(self, plan: Plan, device, buckets: Sequence[int]):
        self.plan = plan
        self.device = K.as_device(device)
        self.buckets = sorted(set(int(b) for b in buckets))
        B = self.buckets[-1]
        self.step_out: List[torch.Tensor] = []
        self.tree_partial: Optional[torch.Tensor] = None
        self.tree_groups: Dict[int, int] = {}
        steps = plan.steps
        self.consumers = step_consumers(steps)
        for i, s in enumerate(steps):
            last = i == len(steps) - 1
            cons = self.consumers[i]
            feeds_mma = (not last) and bool(cons) and all(steps[j].kind in ("dense", "head", "join", "row", "quant")
                                                          for j in cons)
            # bf16 plans hand bf16 activations to the MFMA layers reading them (joins, row steps and
            # QuantizeLinear pass them on / read them in the same dtype); fp32 plans stay f32
            # (a column step reads f32 only, so whatever feeds one stays f32; its own output follows the rule)
            dt = (torch.bfloat16 if (s.kind in ("dense", "qdense", "dequant", "gru", "lstm", "join", "row", "cols")
                                     and feeds_mma and plan.precision == "bf16")
                  else torch.float32)
            if s.kind in ("conv", "seqpool") and not last:
                # TcnModel owns these steps' buffers; a placeholder keeps step_out indexed by step
                self.step_out.append(torch.zeros((0, s.out_width), dtype=torch.float32, device=self.device))
            elif step_qtype(s) is not None:
                # quantised bytes: rows padded to 16 so qgemm loads and stores them as 16-byte vectors
                self.step_out.append(torch.zeros((B, -(-s.out_width // 16) * 16), dtype=torch.int8, device=self.device))
            else:
                self.step_out.append(torch.zeros((B, s.out_width), dtype=dt, device=self.device))
            if s.kind == "tree":
                need = 0
                for b in self.buckets:
                    g = tree_groups(s, b)
                    self.tree_groups[b] = g
                    need = max(need, g * b * s.k)
                self.tree_partial = torch.zeros(max(need, 1), dtype=torch.float32, device=self.device)
        # tree -> head pairs that run as one launch (trees.hip tree_head_kernel) need one ticket
        # counter per 64-row tile (the kernel returns them to zero)
        self.tile_cnt = torch.zeros(-(-B // 64), dtype=torch.int32, device=self.device)
        # sequence models: the GRU layers (+ an N=1 head) run as ONE fused K4 launch
        # (a bidirectional layer: two launches + the head, GruModel / LstmModel; the attribute
        # keeps its name for either cell)
        self.gru = None
        self.gru_steps = 0
        if has_sequence(steps):
            self.gru = sequence_model(steps, self.device, plan.precision != "bf16", B)
            self.gru_steps = len(steps)
            self.seq_len = steps[0].seq
        self.out = self.step_out[-1] if self.step_out else None

    @property
    def out_width(self) -> int:
        return self.plan.out_width

    def fuses_ensemble(self, bucket: Optional[int] = None) -> bool:
        """Whether :meth:`run` can run the scorer's K5 ensemble in the epilogue of its last step:
        an N=1 MLP head whose output column is the model score, or (for ``bucket``) a
        complete-layout tree ensemble as the only step, launched in groups, whose finish kernel
        then runs K5 (IGP_FUSE_TREE_ENS=0 keeps the standalone ensemble there)."""
        steps = self.plan.steps
        if self.gru is not None or not steps:
            return False
        if steps[-1].kind == "head":
            return self.plan.ml_col == 0
        return (bucket is not None and len(steps) == 1 and steps[0].kind == "tree"
                and steps[0].layout != "sparse" and self.tree_groups.get(bucket, 1) > 1
                and os.environ.get("IGP_FUSE_TREE_ENS", "1") != "0")

    def run(self, X: torch.Tensor, bucket: int, m_ptr: Optional[torch.Tensor] = None,
            ens: Optional[dict] = None, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """X: [rows, in] f32 (or [T, rows, I] for a GRU model); returns the last step's buffer.
        ``ens`` (only when :meth:`fuses_ensemble`): K5 arguments for the fused head epilogue.
        ``lens``: int32 [rows] sequence lengths for a plan with ``lens_input`` (None: full length)."""
        steps = self.plan.steps
        if ens is not None and not self.fuses_ensemble(bucket):
            raise ValueError("this plan cannot fuse the ensemble")
        if lens is not None and self.gru is None:
            raise ValueError("lens given, but the model is no sequence model")
        if self.gru is not None:
            if self.plan.steps[0].layout == 1:  # batch-major model input [rows, T, I]
                X = X.transpose(0, 1).contiguous()
            if lens is not None and self.plan.lens_input is None:
                raise ValueError("lens given, but the model has no sequence_lens input")
            self.gru.run(bucket, X.shape[0], self.out, X=X, m_ptr=m_ptr, lens=lens)
            return self.out
        cur = X
        fused_partial = None
        skip = -1
        one_launch = os.environ.get("IGP_TREE_HEAD", "1") != "0"

        def value(k):
            return X if k < 0 else self.step_out[k]
        for i, (s, out) in enumerate(zip(steps, self.step_out)):
            if i == skip:
                cur = out
                continue
            if s.kind == "join":  # two branches of a DAG model meet
                K.join(s.op, value(s.a), value(s.b), out, bucket, s.na, s.nb, m_ptr=m_ptr)
                fused_partial = None
                cur = out
                continue
            cur = value(step_inputs(steps, i)[0])
            if s.kind == "tree" and s.layout == "sparse":
                K.tree_sparse(s, cur, out, bucket, partial=self.tree_partial, groups=self.tree_groups.get(bucket, 1))
                fused_partial = None
            elif s.kind == "tree":
                g = self.tree_groups.get(bucket, 1)
                fuse = (g > 1 and i + 1 < len(steps) and steps[i + 1].kind == "head" and s.post == 0
                        and s.binary_class < 0 and steps[i + 1].k == s.k and self.consumers[i] == [i + 1]
                        and step_inputs(steps, i + 1) == (i,))
                if fuse and one_launch and K.tree_head_ok(s, steps[i + 1], g):
                    # the head (and the K5 of a last head) in the tree kernel's last-arriving blocks
                    K.tree_head(s, steps[i + 1], cur, self.step_out[i + 1], bucket, self.tree_partial, g,
                                self.tile_cnt, m_ptr=m_ptr, ens=ens if i + 1 == len(steps) - 1 else None)
                    skip = i + 1
                    cur = out
                    continue
                K.tree_ensemble(s, cur, None if fuse else out, bucket, partial=self.tree_partial,
                                groups=g, no_finish=fuse, ens=ens if i == len(steps) - 1 else None)
                fused_partial = (self.tree_partial, g, s) if fuse else None
            elif s.kind == "row":  # layernorm / softmax / an activation with no dense layer to ride on
                K.row_op(s.op, cur, out, bucket, s.width, act=s.act, p0=s.p0, p1=s.p1, eps=s.eps, gamma=s.gamma,
                         beta=s.beta, m_ptr=m_ptr)
                fused_partial = None
            elif s.kind == "cols":  # a ColumnTransformer front end: one launch assembles the estimator's input
                K.col_assemble(s, cur, out, bucket, m_ptr=m_ptr)
                fused_partial = None
            elif s.kind == "dense":
                K.dense(cur, s.w, s.b, out, bucket, s.n, s.k, act=s.act, m_ptr=m_ptr)
            elif s.kind == "qdense":  # int8 MFMA on the quantised bytes of the producing step
                K.qdense(cur, s.w8, s.corr, s.mult, s.b, out, bucket, s.n, s.k, act=s.act, out_q=s.out_q, m_ptr=m_ptr)
            elif s.kind == "svm":  # kernel machine on the f32 matrix cores, whatever the plan's precision
                K.svm(s, cur, out, bucket, m_ptr=m_ptr)
            elif s.kind == "quant":
                K.quantize(cur, out, bucket, s.width, s.scale, s.zp, s.qtype, m_ptr=m_ptr)
            elif s.kind == "dequant":
                K.dequantize(cur, out, bucket, s.width, s.scale, s.zp, s.qtype, m_ptr=m_ptr)
            elif s.kind == "head":
                K.mlp_head(s, cur, out, bucket, m_ptr=m_ptr, tree_partial=fused_partial,
                           ens=ens if i == len(steps) - 1 else None)
                fused_partial = None
            cur = out
        return cur
