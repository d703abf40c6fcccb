#!/usr/bin/env python3
"""K4 GRU tile sweep: rows per workgroup x waves per workgroup x batch, event-ring input
(cfg 5 model: 2x256, T=100, I=16). Checks that every variant gives the same scores.
GRU_MASKED=1: the batch-parallel variants also as masked (ONNX sequence_lens) instances, timed in
alternation with their unmasked twins; their windows come from ev_count, so short rings score
differently (max_diff_vs_first is then no check)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    import torch
    from igaming_platform_amd.utils import benchkit
    from igaming_platform_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    S = benchkit.build_model("cfg5", 8192, 1 << 18, dev, use_graphs=False)
    R = S.runner
    res = []
    ref = {}
    batches = [int(b) for b in os.environ.get("GRU_BATCHES", "512,4096,8192").split(",")]
    variants = ((16, 0, 1, 1), (16, 0, 1, 3), (16, 4, 0, 0), (16, 8, 0, 0), (32, 4, 0, 0), (16, 0, 1, 0), (32, 0, 1, 0))
    if os.environ.get("GRU_WS_ONLY"):  # the cluster kernels and the default batch-parallel one
        variants = ((16, 0, 1, 1), (16, 0, 1, 3), (16, 0, 1, 0))
    masked_gp = None
    if os.environ.get("GRU_MASKED"):
        import copy
        masked_gp = copy.copy(R.gp)   # the same device weights; the masked kernels, no cluster workspace
        masked_gp.masked, masked_gp.ws_ok, masked_gp.wsx_ok = True, False, False
        variants = tuple(v for v in variants if v[3] == 0)
    for B in batches:
        slots = torch.from_numpy(np.random.default_rng(B).integers(0, 1 << 18, B).astype(np.int32)).to(dev)
        for tr, w, pipe, ws in variants:
            packs = [(False, R.gp)] + ([(True, masked_gp)] if masked_gp is not None else [])
            outs = {m: torch.zeros(B, device=dev) for m, _ in packs}
            runs = {m: (lambda gp=gp, m=m: K.gru(gp, B, R.T, out=outs[m], store=R.store, slots=slots, tile_rows=tr,
                                                 waves=w, pipeline=pipe, ws=ws)) for m, gp in packs}
            ts = {m: [] for m in runs}
            for m, run in runs.items():
                run()
            torch.cuda.synchronize()
            if B not in ref:
                ref[B] = outs[False].clone()
            for _ in range(3 if masked_gp is not None else 1):  # alternate the packs in the same process
                for m, run in runs.items():
                    for _ in range(10):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run()
                        e1.record()
                        e1.synchronize()
                        ts[m].append(e0.elapsed_time(e1))
            for m in runs:
                ms = float(np.median(ts[m][2:]))
                r = dict(batch=B, ws=ws, tile_rows=tr, waves=w, pipeline=pipe, masked=m, ms=ms, ms_min=float(min(ts[m][2:])),
                         ms_max=float(max(ts[m][2:])), seq_per_s=B / ms * 1e3, us_per_step=ms * 10,
                         max_diff_vs_first=float((outs[m] - ref[B]).abs().max()), ws_failed=R.gp.ws_failed())
                res.append(r)
                print(json.dumps(r), flush=True)
    with open(os.environ.get("OUT", "gpurun_out/gru_sweep.json"), "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
