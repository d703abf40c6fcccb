"""GPU scoring pipeline for one MI355X (one feature shard, one model replica).

One micro-batch = three captured hipGraphs on three HIP streams:

  copy stream
    H2D  pinned slab [BatchHdr | ReqRec x n] -> the slot's device slab      (one copy)
    K6a  dedup insert: the batch's accounts -> its dedup ring region, with per-account row
         lists and the list of accounts with several events in the batch
  state stream (owns the HBM feature store; batches run strictly in submit order)
    K1   feature_assemble (+blacklist, +ip-intel, +HLL counts, +rules) -> X, FeatRec, then
         score-then-update of every account with one event in the batch
    K6b  update_multi: the multi-event accounts' events in row order (one wave each), then
         clear the dedup region of batch seq+7 (eight-region ring, launch.h DEDUP_RING)
  model stream (reads only the slot's X / FeatRec; never touches the store)
    K2/K3 model steps of the compiled ONNX plan                            -> ml
    K5   ensemble + action (+K10 metrics histogram)                        -> ResultRec
    D2H  ResultRec [n] -> pinned result buffer                             (one copy)

Score-then-update (engine.go:486-488) needs only the batch's own requests and the state K1
read, so the whole store read-modify-write finishes in the state graph, and the next batch's
K1 starts while this batch's trees / MLP / ensemble still run on the model stream; its copy
and dedup insert run even earlier, under this batch's K1 (dedup regions rotate over eight by
batch seq; the state graph of batch q clears the region of batch q+7, so the copy of batch q
needs the state graph of batch q-7: the native driver keeps one event per ring entry, this
Python path waits for batch q-2's, which covers it). Each pipeline slot has its own device slab, X,
FeatRec, result and model activation buffers; a slot is reused only after the model graph
that last read it.

Graphs are captured per (batch bucket, pipeline slot); a batch is padded to the smallest
bucket >= n and kernels read the live count and the clock from the device header, so padded
rows are inert and ReqRec.ts is ignored (every request of a batch happens at its ``now``).
Thresholds/weights live in a device config block (``cfg_dev``): UpdateThresholds is a
176-byte copy, never a re-capture. Pipeline slots multi-buffer the pinned host memory so the
host packs batch i+1 while the GPU runs batch i.
"""
from __future__ import annotations

import collections
import os
import threading
import time
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np
import torch

from ..config import Config
from ..layouts import (BATCHHDR, FEATREC, MODEL_HEURISTIC, MODEL_NONE, MODEL_OUTPUT, REQREC, score_cfg,
                       unpack_results)
from ..models.plan import Plan, has_sequence
from ..ops import kernels as K
from .runner import DeviceModel

HDR_BYTES = 16
REQ_BYTES = REQREC.itemsize
_CU_STREAMS: Dict[tuple, tuple] = {}  # (device, split) -> CU-masked (state, copy, model) streams


def _destroy_cu_streams() -> None:
    """Interpreter exit: drain and destroy the CU-masked streams while the HIP runtime (and a
    profiler attached to it) is still up, instead of leaving them to runtime teardown."""
    import torch
    for key, streams in list(_CU_STREAMS.items()):
        try:
            for st in streams:
                st.synchronize()
                K._mod().cu_stream_destroy(st.cuda_stream)
        except Exception:  # best effort at exit
            pass
    _CU_STREAMS.clear()


_FEAT_ENC = os.environ.get("IGP_FEAT_ENC", "1") != "0"
# K1 stores each row's 128-B feature image straight into the slot's pinned host buffer (one
# coalesced store per row through the fabric) instead of device memory + a D2H copy on the model
# stream: that copy ran as a 20 us blit kernel per serving step. The
# exchange scorer (engine/dp.py) keeps the device image: its all-to-all sends it to the sender.
_FEAT_HOST = os.environ.get("IGP_FEAT_HOST", "1") != "0"

class _Slot:
    """Device buffers of one pipeline slot (slab, model input/output, results)."""


@dataclass
class Pending:
    slot: int
    n: int
    bucket: int
    event: "torch.cuda.Event"
    t_submit: float
    want_features: bool
    keep: Any = None   # request rows the native driver still reads (asynchronous issue)


class GpuScorer:
    fenc_to_host = _FEAT_HOST  # K1 writes the D2H feature images into host_feat[slot] directly

    def __init__(self, cfg: Config, store, plan: Optional[Plan] = None, model: str = "plan",
                 device=None, pipeline_depth: int = 2, update_features: bool = True,
                 use_graphs: Optional[bool] = None, owner_filter: bool = False, rank: int = 0):
        self.cfg = cfg
        # _native.StateClock of the shard (engine/backends.py): the driver publishes each batch's
        # state-stage event into it, feature-store readers wait on it (csrc/kernels/state_clock.h)
        self.state_clock = None
        # broadcast serving (multi-GPU): every rank sees the whole batch, scores only the rows
        # whose owner byte (ReqRec.tx_type bits 8-15) is its rank, zeroes the rest
        self.owner_filter = bool(owner_filter)
        self.rank = int(rank)
        self.store = store
        self.device = K.as_device(device) if device is not None else store.device
        self.plan = plan
        if plan is None and model == "plan":
            model = "none"
        self.model = model
        self.update_features = update_features
        self.direct = False
        self.use_graphs = cfg.gpu.use_graphs if use_graphs is None else use_graphs
        self.buckets = sorted(set(int(b) for b in cfg.gpu.buckets))
        self.bmax = self.buckets[-1]
        if store.dmax < self.bmax:
            raise ValueError("store.max_events must cover the largest bucket (score-then-update)")
        self.width = cfg.features.width
        if plan is not None and plan.in_width > 0 and plan.in_width != self.width:
            raise ValueError(f"model input width {plan.in_width} != features.width {self.width}")
        dev = self.device
        B = self.bmax
        self.slab_bytes = HDR_BYTES + REQ_BYTES * B
        self.depth = int(pipeline_depth)
        # the pinned slab of a slot: [BatchHdr | ReqRec x B | segment table]. The table (device_ops.h
        # IgpRowSegTable, 16-byte aligned behind the rows) is the serving core's: with a live count
        # in it the dedup insert reads the step's rows from the requests' own pinned buffers
        # instead of the slab (cfg.gpu.inplace_rows); zero, as every other submitter leaves it,
        # means the rows are in the slab
        self.inplace_rows = bool(getattr(cfg.gpu, "inplace_rows", True))
        host_bytes = self.slab_bytes + K.ROW_SEG_TABLE_BYTES
        self.host_slab = [torch.zeros(host_bytes, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self.host_segs = [t[self.slab_bytes:] for t in self.host_slab]
        self.host_slab_np = [t.numpy() for t in self.host_slab]
        self.host_res = [torch.zeros((B, 2), dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self.host_feat = [torch.zeros((B, 32), dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        # numpy views of the pinned result rows: wait() slices these (a torch slice + .numpy()
        # per batch cost ~3 us of host time on the issue thread)
        self._host_res_np = [t.numpy() for t in self.host_res]
        self._host_feat_np = [t.numpy() for t in self.host_feat]
        self.slots = [self._alloc_slot() for _ in range(self.depth)]
        self._cur = 0  # slot of the last submitted batch (the un-indexed buffer properties)
        self.metrics = torch.zeros(128, dtype=torch.int64, device=dev)
        # equal stream priorities: a high-priority state, model or copy stream measured the same
        # (round-5 A/B, profiles/r5/eng/prio)
        self.stream = torch.cuda.Stream(device=dev)    # state stream (feature store owner)
        # H2D + dedup insert beside K1 (in order on the state stream instead: 78 vs 100 M
        # scores/s, profiles/NOTES.md "Model stream")
        self.cstream = torch.cuda.Stream(device=dev)
        self.mstream = torch.cuda.Stream(device=dev)   # model / result stream
        # state/copy streams and the model stream on disjoint CU halves (CU-masked HIP streams):
        # K1 and the tree/MLP kernels slowed each other 2-7x when sharing CUs (rocprofv3
        # timeline); same-box A/B cfg3 109.1 vs 97.5 M scores/s (3 runs each, profiles/NOTES.md).
        # Only with a model plan: the heuristic model stream is just the ensemble.
        split = os.environ.get("IGP_CU_SPLIT", "auto")
        if split == "auto":
            # With direct launch the masks no longer pay (same-box A/Bs, 3000-step runs: no split
            # 107.6 vs half 101.8 M scores/s, 5 x 600 steps on another box: median 130.5 vs 127.5;
            # profiles/r2/cu, cu3): they were a win for the graph-replay pipeline only
            direct = self.use_graphs and os.environ.get("IGP_NATIVE_DRIVER", "1") != "0" and self._direct_default()
            split = "half" if plan is not None and not direct else "none"
        if split != "none":
            self._cu_split(split)
        self._copy_ev = [torch.cuda.Event() for _ in range(self.depth)]
        self._state_ev = [torch.cuda.Event() for _ in range(self.depth)]
        self._model_ev = [torch.cuda.Event() for _ in range(self.depth)]
        self._state_hist: collections.deque = collections.deque(maxlen=2)  # state events, batch order
        self.cfg_dev = torch.zeros(176, dtype=torch.uint8, device=dev)
        self.refresh_config()
        self.graphs: Dict[tuple, tuple] = {}
        self._host_results = True  # K5 writes the result rows straight into pinned host memory
        self.driver = None
        self._slot = 0
        self._seq = 0
        self._lock = threading.Lock()
        self.batches = 0

    @staticmethod
    def _direct_default() -> bool:
        """Whether this pipeline issues its stages by direct launch (the exchange scorer keeps
        graph replay by default and overrides this)."""
        return os.environ.get("IGP_DIRECT_LAUNCH", "1") == "1"

    def _cu_split(self, spec: str) -> None:
        """``half`` = ``lo:n_cu/2``; ``lo:N``: CUs [0, N) run the copy + state streams, the
        rest the model stream; ``mod:A/B``: CU i goes to the state side when i % B < A."""
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        if spec == "half":
            spec = f"lo:{n_cu // 2}"
        kind, arg = spec.split(":")
        if kind == "lo":
            st = [i < int(arg) for i in range(n_cu)]
        else:
            a, b = (int(x) for x in arg.split("/"))
            st = [i % b < a for i in range(n_cu)]

        def words(sel):
            w = [0] * ((n_cu + 31) // 32)
            for i, on in enumerate(sel):
                if on:
                    w[i // 32] |= 1 << (i % 32)
            return w

        model = [not x for x in st]
        key = (self.device.index, kind, arg)
        if key not in _CU_STREAMS:  # HIP streams live for the process: reused by later scorers
            masks = (st, st, model)
            with torch.cuda.device(self.device):
                _CU_STREAMS[key] = tuple(torch.cuda.ExternalStream(K._mod().cu_stream(words(m)), device=self.device)
                                         for m in masks)
            if len(_CU_STREAMS) == 1:
                import atexit
                atexit.register(_destroy_cu_streams)
        self.stream, self.cstream, self.mstream = _CU_STREAMS[key]

    # ------------------------------------------------------------------ buffers / config
    def _alloc_slot(self) -> "_Slot":
        dev, B = self.device, self.bmax
        sb = _Slot()
        sb.dev_slab = torch.zeros(self.slab_bytes, dtype=torch.uint8, device=dev)
        sb.hdr = sb.dev_slab[:HDR_BYTES].view(torch.int64)
        sb.n_ptr = sb.dev_slab[:4].view(torch.int32)
        sb.req = sb.dev_slab[HDR_BYTES:]
        sb.X = torch.zeros((B, self.width), dtype=torch.float32, device=dev)
        sb.feat = torch.zeros((B, 32), dtype=torch.int32, device=dev)
        # the rows' 128-B D2H feature images: K1 writes the raw FeatRec, or the encoded risk.v1
        # FeatureVector body for rows the serving core marked (FV_ENC_BIT: its response writer
        # then copies bytes instead of serialising 26 fields per row). IGP_FEAT_ENC=0: raw only
        sb.fenc = torch.zeros((B, 32), dtype=torch.int32, device=dev) if _FEAT_ENC else None
        sb.res = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        sb.model = None
        if self.plan is not None:
            if has_sequence(self.plan.steps):
                raise ValueError("fraud scoring models take a feature vector; sequence models (GRU / LSTM) run in "
                                 "the abuse scorer")
            sb.model = DeviceModel(self.plan, dev, self.buckets)
        return sb

    # buffers of the last submitted batch (tests / tools)
    X = property(lambda self: self.slots[self._cur].X)
    feat = property(lambda self: self.slots[self._cur].feat)
    res = property(lambda self: self.slots[self._cur].res)
    hdr = property(lambda self: self.slots[self._cur].hdr)
    req = property(lambda self: self.slots[self._cur].req)
    n_ptr = property(lambda self: self.slots[self._cur].n_ptr)
    dev_slab = property(lambda self: self.slots[self._cur].dev_slab)
    model_dev = property(lambda self: self.slots[self._cur].model)
    ml = property(lambda self: self.slots[self._cur].model.out if self.slots[self._cur].model else None)
    step_out = property(lambda self: self.slots[self._cur].model.step_out if self.slots[self._cur].model else [])
    tree_partial = property(lambda self: self.slots[self._cur].model.tree_partial
                            if self.slots[self._cur].model else None)
    tree_groups = property(lambda self: self.slots[self._cur].model.tree_groups
                           if self.slots[self._cur].model else {})

    def refresh_config(self, scoring=None) -> None:
        """Write the device config block (thresholds, weights, table sizes). The last
        ``scoring`` given stays in force for later refreshes (e.g. a blacklist sync)."""
        if scoring is not None:
            self.scoring = scoring
        scoring = getattr(self, "scoring", None) or self.cfg.scoring
        kind = {"none": MODEL_NONE, "heuristic": MODEL_HEURISTIC, "plan": MODEL_OUTPUT}[self.model]
        ml_col = self.plan.ml_col if self.plan is not None else 0
        ml_stride = self.plan.out_width if self.plan is not None else 1
        c = score_cfg(self.cfg, kind, ml_col=ml_col, ml_stride=ml_stride, sc=scoring,
                      owner_filter=self.owner_filter, my_rank=self.rank, **self.store.table_params())
        self.store.sync_tables()
        # batches already on the model stream finish under the config they were submitted with
        torch.cuda.current_stream(self.device).wait_stream(self.mstream)
        self.cfg_dev.copy_(torch.from_numpy(c.view(np.uint8).copy()))

    # ------------------------------------------------------------------ the step
    def _copy_body(self, slot: int, bucket: int) -> None:
        sb = self.slots[slot]
        if self.update_features:
            # the dedup insert reads the batch from the pinned slab and writes the device copy (an
            # H2D copy first and the insert from HBM: same engine_only / serving, round-5 A/B
            # profiles/r5/eng/dedup_src)
            K.dedup_insert(self.store, self.cfg_dev, sb.req, bucket, sb.hdr, src=self.host_slab[slot],
                           segs=self.host_segs[slot])
            return
        K.memcpy_async(sb.dev_slab, self.host_slab[slot], HDR_BYTES + REQ_BYTES * bucket)

    def _state_body(self, slot: int, bucket: int, part: str = "all") -> None:
        """K1 (part "k1"), which also clears the dedup region of batch seq + DEDUP_AHEAD, then the
        multi-event update (part "update"). Part "k1own": the K1 that scores and applies the short
        multi-event accounts itself, for batches the native driver issues without the update."""
        sb, upd = self.slots[slot], self.update_features
        if part in ("all", "k1", "k1own"):
            route = self._fenc_route(slot, bucket)
            K.feature_assemble(self.store, sb.hdr, self.cfg_dev, sb.req, sb.X, sb.feat, bucket, dedup=upd,
                               own_short=upd and part == "k1own",
                               fenc=None if route is not None else self._fenc_out(slot), fenc_route=route)
        if upd and part in ("all", "update"):
            K.update_segments(self.store, self.cfg_dev, sb.req, bucket, sb.hdr)

    def _model_body(self, slot: int, bucket: int, with_features: bool = False) -> None:
        sb = self.slots[slot]
        # K5 writes the result rows straight into the slot's pinned host buffer as well (no
        # D2H copy node on the model stream)
        host = self.host_res[slot] if self._host_results else None
        if sb.model is not None and sb.model.fuses_ensemble(bucket):
            # K5 in the MLP head's (or the grouped trees' finish kernel's) epilogue: one launch fewer
            ens = K.ensemble_args(sb.hdr, self.cfg_dev, sb.feat, sb.X, sb.model.step_out[-1], sb.res, bucket,
                                  self.metrics, host_out=host)
            sb.model.run(sb.X, bucket, m_ptr=sb.n_ptr, ens=ens)
        else:
            ml = sb.model.run(sb.X, bucket, m_ptr=sb.n_ptr) if sb.model is not None else None
            K.ensemble(sb.hdr, self.cfg_dev, sb.feat, sb.X, ml, sb.res, bucket, self.metrics, host_out=host)
        if host is None:
            K.memcpy_async(self.host_res[slot], sb.res, bucket * sb.res[0].numel() * sb.res.element_size())
        if with_features and not self._fenc_host():
            img = sb.fenc if sb.fenc is not None else sb.feat
            K.memcpy_async(self.host_feat[slot], img, bucket * img[0].numel() * img.element_size())

    def _fenc_host(self) -> bool:
        return self.fenc_to_host and _FEAT_ENC

    def _fenc_route(self, slot: int, bucket: int):
        """K1 writes the feature images straight into their senders' chunks of a results region
        (engine/dp.py, the rows-region exchange); None here."""
        return None

    def _fenc_out(self, slot: int):
        """Where K1 writes the slot's feature images: the pinned host rows (default) or the
        slot's device buffer (copied by the model stage when features are requested)."""
        return self.host_feat[slot] if self._fenc_host() else self.slots[slot].fenc

    def capture(self) -> None:
        """Capture the copy, state, model and model+features graphs per (bucket, pipeline
        slot); each body runs once eagerly first (n = 0). With the native driver
        (csrc/kernels/driver.hip, default) every later submit is issued from C++."""
        if not self.use_graphs:
            return
        # Each body is captured on the stream it replays on: HIP multiplexes streams onto
        # GPU_MAX_HW_QUEUES (4) hardware queues, and throwaway capture streams shifted the copy
        # and model streams onto ONE queue, which serialised the pipeline (rocprofv3 queue ids).
        # With the default stream plus these three, every stream owns a queue.
        with torch.cuda.device(self.device):
            for b in self.buckets:
                for slot in range(self.depth):
                    self._write_hdr(slot, 0, 0)
                    pair = []
                    for body, s in ((lambda: self._copy_body(slot, b), self.cstream),
                                    (lambda: self._state_body(slot, b), self.stream),
                                    (lambda: self._model_body(slot, b), self.mstream),
                                    (lambda: self._model_body(slot, b, with_features=True), self.mstream)):
                        s.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(s):
                            body()
                        torch.cuda.current_stream().wait_stream(s)
                        g = torch.cuda.CUDAGraph()
                        with K.graph_capture(g, s):
                            body()
                        pair.append(g)
                    self.graphs[(b, slot)] = tuple(pair)
            torch.cuda.synchronize(self.device)
        self.driver = None
        if os.environ.get("IGP_NATIVE_DRIVER", "1") != "0":
            d = K._mod().PipeDriver(self.cstream.cuda_stream, self.stream.cuda_stream, self.mstream.cuda_stream,
                                    self.depth, [t.data_ptr() for t in self.host_slab])
            for slot in range(self.depth):  # what the native serving core reads after a wait
                d.set_host_results(slot, self.host_res[slot].data_ptr(), self.host_feat[slot].data_ptr())
                if self.inplace_rows and self.update_features:  # (the plain H2D copy stage reads the slab only)
                    d.set_row_segs(slot, self.host_segs[slot].data_ptr())
            if self.state_clock is not None:
                d.set_state_clock(self.state_clock)
            for (b, slot), g in self.graphs.items():
                d.set_graphs(b, slot, g[0].raw_cuda_graph_exec(), g[1].raw_cuda_graph_exec(),
                             g[2].raw_cuda_graph_exec(), g[3].raw_cuda_graph_exec())
            # direct launch (csrc/kernels/oplist.h): the stages' kernels issued as plain launches
            # instead of graph replays (a graph launch costs ~7 us of queue time on MI355X)
            self.direct = (os.environ.get("IGP_DIRECT_LAUNCH", "1") == "1"
                           and not has_sequence(self.plan.steps if self.plan else []))
            if self.direct:
                with torch.cuda.device(self.device):
                    for b in self.buckets:
                        for slot in range(self.depth):
                            # the state stage split in two (IGP_SPLIT_STATE, default on): the
                            # model waits for K1 only, the multi-event update runs beside it
                            split = os.environ.get("IGP_SPLIT_STATE", "1") == "1"
                            lists = []
                            for body in (lambda: self._copy_body(slot, b),
                                         lambda: self._state_body(slot, b, "k1" if split else "all"),
                                         lambda: self._model_body(slot, b),
                                         lambda: self._model_body(slot, b, with_features=True),
                                         lambda: self._state_body(slot, b, "update"),
                                         lambda: self._state_body(slot, b, "k1own")):
                                with K.Recorder() as r:
                                    body()
                                lists.append(r.ops)
                            d.set_ops(b, slot, *lists[:4])
                            if split:
                                d.set_state_update(b, slot, lists[4], lists[5])
            # (round 5 removed the one-stream serial mode - cfg2 22.6 vs 11.0 M, cfg3 107 vs 57 M,
            # profiles/r2/serial - and the asynchronous issue thread - cfg3 118 vs 127 M,
            # profiles/r2/direct3: both measured slower)
            self.driver = d

    def bucket_for(self, n: int) -> int:
        for b in self.buckets:
            if n <= b:
                return b
        raise ValueError(f"batch of {n} exceeds the largest bucket {self.bmax}")

    def _write_hdr(self, slot: int, n: int, now: int) -> None:
        h = self.host_slab_np[slot][:HDR_BYTES].view(BATCHHDR)
        h["n"] = n
        h["seq"] = self._seq
        h["now"] = now

    def slab_view(self, slot: int, n: int) -> np.ndarray:
        return self.host_slab_np[slot][HDR_BYTES:HDR_BYTES + REQ_BYTES * n].view(REQREC)

    def next_slot(self) -> int:
        with self._lock:
            s = self._slot
            self._slot = (self._slot + 1) % self.depth
        return s

    def submit_packed(self, slot: int, n: int, now: int, want_features: bool = False,
                      rows: Optional[np.ndarray] = None) -> Pending:
        """Launch a batch whose ReqRec rows are already in ``slab_view(slot, n)`` (or, with the
        native driver, are copied from ``rows`` by it)."""
        b = self.bucket_for(max(n, 1))
        self._seq += 1
        t0 = time.perf_counter()
        if self.driver is not None:
            if rows is not None:
                rows = np.ascontiguousarray(rows)
            self.driver.submit(slot, b, n, self._seq, int(now), 0 if rows is None else rows.ctypes.data,
                               bool(want_features))
            self._cur = slot
            self.batches += 1
            return Pending(slot, n, b, None, t0, want_features, keep=rows)
        if rows is not None:
            self.pack(slot, rows)
        self._write_hdr(slot, n, now)
        g = self.graphs.get((b, slot))
        with torch.cuda.stream(self.cstream):
            self.cstream.wait_event(self._model_ev[slot])  # the slot's device buffers are free
            # batch seq-3's state stage cleared this batch's dedup region; seq-2's comes after it
            if len(self._state_hist) == 2:
                self.cstream.wait_event(self._state_hist[0])
            if g is not None:
                g[0].replay()
            else:
                self._copy_body(slot, b)
            self._copy_ev[slot].record(self.cstream)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(self._copy_ev[slot])
            if g is not None:
                g[1].replay()
            else:
                self._state_body(slot, b)
            sev = torch.cuda.Event()
            sev.record(self.stream)
        self._state_ev[slot] = sev
        self._state_hist.append(sev)
        with torch.cuda.stream(self.mstream):
            self.mstream.wait_event(sev)
            if g is not None and not want_features:
                g[2].replay()
            else:
                self._model_body(slot, b, with_features=want_features)
            ev = torch.cuda.Event()
            ev.record(self.mstream)
        self._model_ev[slot] = ev
        self._cur = slot
        self.batches += 1
        return Pending(slot, n, b, ev, t0, want_features)

    def pack(self, slot: int, req: np.ndarray) -> int:
        """Copy REQREC rows into the slot's pinned slab as raw bytes (a field-wise structured
        copy costs ~20x more). Row ``ts`` is ignored on this path: kernels use the batch clock."""
        n = len(req)
        if req.dtype != REQREC:
            req = np.asarray(req, REQREC)
        src = np.ascontiguousarray(req).view(np.uint8).reshape(-1)
        np.copyto(self.host_slab_np[slot][HDR_BYTES:HDR_BYTES + REQ_BYTES * n], src)
        return n

    def submit_into(self, slot: int, req: np.ndarray, now: Optional[int] = None,
                    want_features: bool = False) -> Pending:
        now = int(time.time()) if now is None else int(now)
        return self.submit_packed(slot, self.pack(slot, req), now, want_features)

    def submit(self, req: np.ndarray, now: Optional[int] = None, want_features: bool = False) -> Pending:
        """``req``: REQREC structured array (every row is scored and applied at ``now``)."""
        now = int(time.time()) if now is None else int(now)
        slot = self.next_slot()
        return self.submit_packed(slot, self.pack(slot, req), now, want_features)

    def submit_rows(self, slot: int, rows: np.ndarray, now: int) -> Pending:
        """Copy REQREC ``rows`` into the slot's pinned slab and launch (the copy runs in the
        native driver without the GIL when it is active)."""
        if rows.dtype != REQREC:
            rows = np.asarray(rows, REQREC)
        return self.submit_packed(slot, len(rows), now, rows=rows)

    def done(self, p: Pending) -> bool:
        """Non-blocking completion check."""
        return self.driver.query(p.slot) if p.event is None else p.event.query()

    def done_event(self, p: Pending) -> int:
        """Raw hipEvent_t that completes with the batch (the watchdog's deadline wait)."""
        return self.driver.model_event(p.slot) if p.event is None else int(p.event.cuda_event)

    def wait(self, p: Pending, unpack: bool = True):
        if p.event is None:
            self.driver.wait(p.slot)
        else:
            p.event.synchronize()
        res = self._host_res_np[p.slot][:p.n].copy()
        feats = self._host_feat_np[p.slot][:p.n].copy() if p.want_features else None
        if not unpack:
            return res, feats
        out = unpack_results(res)
        if feats is not None:
            out["features"] = feats.view(FEATREC).reshape(-1)
        out["latency_ms"] = (time.perf_counter() - p.t_submit) * 1e3
        return out

    def score(self, req: np.ndarray, now: Optional[int] = None, want_features: bool = False):
        return self.wait(self.submit(req, now, want_features))

    def read_metrics(self, reset: bool = False) -> np.ndarray:
        self.mstream.synchronize()
        m = self.metrics.cpu().numpy().copy()
        if reset:
            self.metrics.zero_()
        return m
