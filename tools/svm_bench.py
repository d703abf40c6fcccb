#!/usr/bin/env python3
"""The kernel-machine step (svm.hip) at 8192 rows for a few (F, S, kernel), one process, runs
interleaved, every row tile.

Every variant is warmed up, then timed ``--reps`` times round-robin with device events around
``--inner`` back-to-back launches; the table gives the median and the 10th / 90th percentile of the
time per launch and the achieved f32 TFLOP/s of the kernel matrix (2 rows S F_pad flops: the MFMAs
run over the padded width; the kernel function and the weighted sum are not counted).
Usage: python tools/svm_bench.py [--rows 8192] [--reps 30] [--inner 10] [--out bench_out/svm_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(30, 512, "RBF"), (30, 4096, "RBF"), (30, 4096, "LINEAR"), (128, 4096, "RBF"), (256, 4096, "RBF"),
          (256, 4096, "POLY"), (256, 4096, "SIGMOID")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default="bench_out/svm_bench.json")
    a = ap.parse_args()
    import torch
    from igaming_platform_amd.models.plan import SVMStep, svm_tables
    from igaming_platform_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("svm_bench: no GPU (nothing is measured on a CPU)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    M = a.rows
    Y = torch.zeros((M, 1), dtype=torch.float32, device=dev)
    variants = []
    for F, S, kern in SHAPES:
        s = SVMStep(kernel=kern, gamma=1.0 / F, coef0=0.5, degree=3, n_sv=S, in_dim=F,
                    sv_np=rng.standard_normal((S, F)).astype(np.float32),
                    coef_np=(rng.standard_normal(S) * 0.1).astype(np.float32),
                    rho=0.1, in_scale=rng.uniform(0.5, 2, F), in_shift=rng.uniform(-0.5, 0.5, F), post_scale=-1.0, act="sigmoid")
        t = svm_tables(s)
        s.sv, s.coef, s.scale, s.shift = (t[k].to(dev) for k in ("sv", "coef", "scale", "shift"))
        s.sv_norm = None if t["sv_norm"] is None else t["sv_norm"].to(dev)
        X = torch.from_numpy(rng.standard_normal((M, F)).astype(np.float32)).to(dev)
        flops = 2.0 * M * S * s.sv.shape[1]
        for tile in (16, 32, 64):
            variants.append((f"svm F={F} S={S} {kern} tile{tile}",
                             (lambda s=s, X=X, tile=tile: K.svm(s, X, Y, M, tile=tile)), flops))
    for _, run, _ in variants:      # warm-up: code objects loaded, clocks up
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {name: [] for name, _, _ in variants}
    for _ in range(a.reps):
        for name, run, _ in variants:
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    res = []
    for name, _, flops in variants:
        t = np.asarray(ts[name])
        r = dict(variant=name, rows=M, picked_tile=K.svm_tile(M), us_median=round(float(np.median(t)), 2),
                 us_p10=round(float(np.percentile(t, 10)), 2), us_p90=round(float(np.percentile(t, 90)), 2),
                 tflops=round(flops / float(np.median(t)) / 1e6, 1))
        res.append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, results=res), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
