#!/usr/bin/env python3
"""K4 LSTM vs GRU timing on one box, one run: 2 x 256 layers + N=1 head, T = 100, I = 16, dense
input, batch-parallel kernels (the GRU with linear_before_reset = 1 and its cluster kernels off),
split (fp32 plans) and bf16 numerics. Median of --iters timed launches after --warmup.
Prints one JSON line per variant and the LSTM / GRU time ratios.
--masked: each variant also as its masked (ONNX sequence_lens) instance with every length T - the
cost of the window test and select alone - timed in rounds that alternate the two."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--seq", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--tile-rows", type=int, default=16, choices=(16, 32))
    ap.add_argument("--masked", action="store_true", help="also time the masked instances (all lengths T), interleaved")
    ap.add_argument("--rounds", type=int, default=4, help="--masked: alternating rounds of --iters launches each")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from igaming_platform_amd.models.plan import compile_onnx
    from igaming_platform_amd.native import native
    from igaming_platform_amd.onnx import builders
    from igaming_platform_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    N = native()
    X = torch.from_numpy(np.random.default_rng(0).standard_normal((a.seq, a.rows, 16)).astype(np.float32)).to(dev)
    out = torch.zeros(a.rows, device=dev)
    res = []
    for cell in ("gru", "lstm"):
        kw = dict(seq=a.seq, in_dim=16, hidden=a.hidden, layers=2, head=True)
        if cell == "gru":
            kw["linear_before_reset"] = 1
        plan = compile_onnx(N.OnnxModel.from_bytes(builders.build(cell, **kw).SerializeToString()))
        layers = [s for s in plan.steps if s.kind == cell]
        for split in (True, False):
            def runner(masked):
                if cell == "gru":
                    pack = K.GruPack(layers, plan.steps[-1], dev, split=split, masked=masked)
                    return lambda: K.gru(pack, a.rows, a.seq, out=out, X=X, tile_rows=a.tile_rows, ws=0)
                pack = K.LstmPack(layers, plan.steps[-1], dev, split=split, masked=masked)
                return lambda: K.lstm(pack, a.rows, a.seq, out=out, X=X, tile_rows=a.tile_rows)

            def timed(run, n):
                ts = []
                for _ in range(n):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1))
                return ts
            runs = {False: runner(False)}
            if a.masked:
                runs[True] = runner(True)
            for run in runs.values():
                for _ in range(a.warmup):
                    run()
            torch.cuda.synchronize()
            ts = {m: [] for m in runs}
            for _ in range(a.rounds if a.masked else 1):  # alternate the two on the same box, same process
                for m, run in runs.items():
                    ts[m] += timed(run, a.iters)
            for m in runs:
                r = dict(cell=cell, mode="split" if split else "bf16", masked=m, rows=a.rows, seq=a.seq, hidden=a.hidden,
                         tile_rows=a.tile_rows, ms_median=float(np.median(ts[m])), ms_min=float(np.min(ts[m])),
                         ms_max=float(np.max(ts[m])), seq_per_s=a.rows / float(np.median(ts[m])) * 1e3,
                         finite=bool(torch.isfinite(out).all()))
                res.append(r)
                print(json.dumps(r), flush=True)
    t = {(r["cell"], r["mode"]): r["ms_median"] for r in res if not r["masked"]}
    ratio = {m: t["lstm", m] / t["gru", m] for m in ("split", "bf16")}
    print(json.dumps(dict(lstm_over_gru=ratio)), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(runs=res, lstm_over_gru=ratio), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
