#!/usr/bin/env python3
"""The column-assembly step (columns.hip) at 8192 rows on a 30 -> 229 column program shaped like a
scikit-learn ColumnTransformer export (10 imputed + standardised, 3 sentinel-imputed + min-max
scaled, 3 categorical columns one-hot encoded to 8 + 193 + 5, 4 binarised, 6 passed through),
against one ``join`` concat that writes the same output bytes. One process, variants interleaved.

Two figures per variant, each the median (p10 - p90) over ``--reps`` windows of ``--inner`` launches
between device events:

* ``graph_us``  the launches captured once in a hipGraph and replayed: no Python between the
                kernels, so this is the kernel plus the graph's node-to-node gap;
* ``eager_us``  the same launches issued from Python: the host's dispatch rate where that is
                slower than the kernel (it is, for kernels this short).

The kernel's own time comes from a kernel trace of this tool (``rocprofv3 --kernel-trace --stats``);
``--only`` narrows the run to the variants whose name contains one of the comma-separated texts, so
that the trace's per-kernel statistics belong to one variant of each kernel.
Usage: python tools/columns_bench.py [--rows 8192] [--reps 30] [--inner 20] [--only TEXT,TEXT] [--out bench_out/columns_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_CAT = (8, 193, 5)


def program():
    """The 30 -> 229 ColumnStep of the module docstring."""
    from igaming_platform_amd.models.plan import ColRec, ColumnStep
    rng = np.random.default_rng(0)
    recs = [ColRec(j, (float("nan"), float(rng.normal())), (float(rng.normal()), float(rng.uniform(0.1, 2)))) for j in range(10)]
    recs += [ColRec(j, (-999.0, float(rng.uniform(20, 80))), (0.0, float(rng.uniform(0.001, 0.01)))) for j in (10, 11, 12)]
    recs += [ColRec(13 + k, None, None, "onehot", float(c)) for k, n in enumerate(N_CAT) for c in range(n)]
    recs += [ColRec(j, None, None, "binarize", 0.5) for j in range(16, 20)]
    recs += [ColRec(j) for j in range(20, 26)]
    return ColumnStep(30, len(recs), recs)


def rows(M):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((M, 30)).astype(np.float32)
    for k, n in enumerate(N_CAT):
        X[:, 13 + k] = rng.integers(0, n, M)
    X[:, :10][rng.random((M, 10)) < 0.1] = np.nan
    X[:, 10:13][rng.random((M, 3)) < 0.1] = -999.0
    return X


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="bench_out/columns_bench.json")
    a = ap.parse_args()
    import torch
    from igaming_platform_amd.models.plan import upload_columns
    from igaming_platform_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("columns_bench: no GPU (nothing is measured on a CPU)", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    M = a.rows
    step = program()
    upload_columns(step, dev)
    W, N = step.in_width, step.out_width
    X30 = torch.from_numpy(rows(M)).to(dev)
    X32 = torch.zeros((M, 32), dtype=torch.float32, device=dev)
    X32[:, :W] = X30
    n4 = -(-N // 4) * 4
    Yf = torch.zeros((M, N), dtype=torch.float32, device=dev)
    Yf4 = torch.zeros((M, n4), dtype=torch.float32, device=dev)
    Yb4 = torch.zeros((M, n4), dtype=torch.bfloat16, device=dev)
    na = N // 2
    A = torch.randn((M, na), dtype=torch.float32, device=dev)
    B = torch.randn((M, N - na), dtype=torch.float32, device=dev)
    variants = [
        (f"col_assemble {W}->{N} ldx {W} f32 ldy {N}", lambda: K.col_assemble(step, X30, Yf, M), M * N * 4),
        (f"col_assemble {W}->{N} ldx 32 f32 ldy {N}", lambda: K.col_assemble(step, X32, Yf, M), M * N * 4),
        (f"col_assemble {W}->{N} ldx 32 f32 ldy {n4}", lambda: K.col_assemble(step, X32, Yf4, M), M * N * 4),
        (f"col_assemble {W}->{N} ldx 32 bf16 ldy {n4}", lambda: K.col_assemble(step, X32, Yb4, M), M * N * 2),
        (f"join concat {na}+{N - na} f32 ldy {N}", lambda: K.join("concat", A, B, Yf, M, na, N - na), M * N * 4),
    ]
    variants = [v for v in variants if any(t in v[0] for t in a.only.split(","))]
    for _, run, _ in variants:      # warm-up: code objects loaded, clocks up
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graphs = {}
    for name, run, _ in variants:   # the inner launches of one window as one graph
        g = torch.cuda.CUDAGraph()
        with K.graph_capture(g, stream):
            for _ in range(a.inner):
                run()
        graphs[name] = g
    torch.cuda.synchronize()
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {(name, how): [] for name, _, _ in variants for how in ("graph", "eager")}
    for _ in range(a.reps):
        for name, run, _ in variants:
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            ts[(name, "graph")].append(e0.elapsed_time(e1) * 1e3 / a.inner)
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            e1.synchronize()
            ts[(name, "eager")].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    res = []
    for name, _, nbytes in variants:
        r = dict(variant=name, rows=M)
        for how in ("graph", "eager"):
            t = np.asarray(ts[(name, how)])
            r.update({f"{how}_us": round(float(np.median(t)), 2), f"{how}_us_p10": round(float(np.percentile(t, 10)), 2),
                      f"{how}_us_p90": round(float(np.percentile(t, 90)), 2)})
        r["out_gb_s_graph"] = round(nbytes / r["graph_us"] / 1e3, 1)
        res.append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, results=res), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
