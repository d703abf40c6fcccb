#!/usr/bin/env python3
"""Per-kernel device time of one scoring step (events around each launch, interleaved rounds
in one process). Usage: python tools/kbench.py [--config cfg3] [--rounds 50]
--config rowops: the row-op kernels alone; --config tcn: conv1d per layer, seq_pool and the head of a
temporal-convolution model, the whole model, and the 2 x 256 GRU beside it."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rowops(rounds: int, out: str) -> None:
    """Device time of every row op (rowops.hip) and of the join add at [8192, 256] and [8192, 2],
    f32, interleaved rounds in one process (``--config rowops``)."""
    import torch
    from igaming_platform_amd.native import hipk
    from igaming_platform_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    M = 8192
    ops = {}
    for N in (256, 2):
        g = torch.Generator(device="cpu").manual_seed(N)
        X = torch.randn((M, N), generator=g).to(dev)
        X2 = torch.randn((M, N), generator=g).to(dev)
        Y = torch.zeros((M, N), device=dev)
        gam, bet = torch.rand(N, generator=g).to(dev) + 0.5, torch.randn(N, generator=g).to(dev)
        ops[f"join_add[{M},{N}]"] = lambda X=X, X2=X2, Y=Y, N=N: K.join("add", X, X2, Y, M, N, N)
        ops[f"layernorm[{M},{N}]"] = lambda X=X, Y=Y, N=N, gam=gam, bet=bet: K.row_op("layernorm", X, Y, M, N,
                                                                                      gamma=gam, beta=bet)
        ops[f"softmax[{M},{N}]"] = lambda X=X, Y=Y, N=N: K.row_op("softmax", X, Y, M, N)
        for act in K.ROW_ACTS:
            p0, p1 = {"clip": (-1.0, 1.0), "selu": (1.6732632, 1.050701), "hard_sigmoid": (0.2, 0.5)}.get(act, (0.1, 0.0))
            ops[f"{act}[{M},{N}]"] = lambda X=X, Y=Y, N=N, act=act, p0=p0, p1=p1: K.row_op("act", X, Y, M, N, act=act,
                                                                                           p0=p0, p1=p1)
    times = {k: [] for k in ops}
    for _ in range(rounds):
        for k, f in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hipk().stall(torch.cuda.current_stream().cuda_stream, 300.0)  # device time only, as in main()
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {k: dict(median_us=float(np.median(v[min(5, len(v) - 1):])), min_us=float(np.min(v[min(5, len(v) - 1):])))
           for k, v in times.items()}
    for k, v in res.items():
        print(f"{k:28s} median {v['median_us']:8.1f} us   min {v['min_us']:8.1f} us")
    if out:
        with open(out, "w") as f:
            json.dump(dict(config="rowops", kernels=res), f, indent=1)


def tcn(rounds: int, out: str, rows: int = 4096) -> None:
    """``--config tcn``: device time of every conv1d launch, the seq_pool and the dense head of the
    typical abuse TCN (4 residual blocks x 64 channels, k = 3, dilations 1 2 4 8, T = 100, 16 inputs)
    at ``rows`` rows, dense input; the whole model (runner.TcnModel.run); and, in the same interleaved
    rounds, the 2 x 256 GRU of cfg5 (runner.GruModel.run, the K4 launch its engine_only path issues:
    fp32 plan = split kernels, and bf16)."""
    import torch
    from igaming_platform_amd.engine.runner import sequence_model
    from igaming_platform_amd.models.plan import compile_onnx, to_device
    from igaming_platform_amd.native import hipk, native
    from igaming_platform_amd.onnx import builders
    from igaming_platform_amd.ops import kernels as K
    dev = torch.device("cuda", 0)
    T = 100
    load = lambda m: native().OnnxModel.from_bytes(m.SerializeToString())
    plan = to_device(compile_onnx(load(builders.tcn(channels=(64,) * 4, dilations=(1, 2, 4, 8)))), dev)
    tm = sequence_model(plan.steps, dev, True, rows)
    X = torch.from_numpy(np.random.default_rng(0).standard_normal((T, rows, 16)).astype(np.float32)).to(dev)
    y = torch.zeros(rows, device=dev)
    ops, flop = {}, 0
    steps, p = tm.steps, tm.n_conv
    for i, s in enumerate(steps[:p]):
        src = s.src if s.src is not None else i - 1
        kw = dict(X=X) if src < 0 else dict(A=tm.bufs[tm.buf_of[src]])
        res = None if s.res is None else tm.bufs[tm.buf_of[s.res]]
        ops[f"conv1d#{i}({s.c_in}->{s.c_out},k={s.k},d={s.dil})"] = (
            lambda s=s, Y=tm.bufs[tm.buf_of[i]], kw=kw, res=res: K.conv1d(s, rows, T, Y, res=res, **kw))
        flop += 2 * s.c_in * s.c_out * s.k * T
    ops["seq_pool(last,64)"] = lambda: K.seq_pool("last", tm.bufs[tm.buf_of[p - 1]], tm.pooled, rows, T, 64)
    ops["seq_pool(mean,64)"] = lambda: K.seq_pool("mean", tm.bufs[tm.buf_of[p - 1]], tm.pooled, rows, T, 64)
    h = steps[-1]
    ops["dense_head(64->1)"] = lambda: K.dense(tm.pooled, h.w, h.b, y.view(-1, 1), rows, 1, h.k, act=h.act)
    ops["tcn_model"] = lambda: tm.run(rows, T, y, X=X)
    for prec in ("fp32", "bf16"):
        gp = to_device(compile_onnx(load(builders.gru(seq=T, in_dim=16, hidden=256, layers=2))), dev, prec)
        gm = sequence_model(gp.steps, dev, prec != "bf16", rows)
        ops[f"gru_2x256_model({prec})"] = lambda gm=gm: gm.run(rows, T, y, X=X)
    times = {k: [] for k in ops}
    for _ in range(rounds):
        for k, f in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hipk().stall(torch.cuda.current_stream().cuda_stream, 300.0)  # device time only, as in main()
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {k: dict(median_us=float(np.median(v[min(5, len(v) - 1):])), min_us=float(np.min(v[min(5, len(v) - 1):])))
           for k, v in times.items()}
    for k, v in res.items():
        print(f"{k:34s} median {v['median_us']:9.1f} us   min {v['min_us']:9.1f} us")
    t_tcn = res["tcn_model"]["median_us"]
    summary = dict(rows=rows, T=T, mflop_per_row=flop / 1e6, tcn_rows_per_s=rows / t_tcn * 1e6,
                   tcn_tflops=flop * rows / t_tcn / 1e6,
                   gru_rows_per_s={p_: rows / res[f"gru_2x256_model({p_})"]["median_us"] * 1e6 for p_ in ("fp32", "bf16")})
    print(json.dumps(summary))
    if out:
        with open(out, "w") as f:
            json.dump(dict(config="tcn", kernels=res, summary=summary), f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", help="a bench config, rowops (the row-op kernels alone) or tcn")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--accounts", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--hot", type=float, default=0.02, help="fraction of requests on 16 hot accounts")
    ap.add_argument("--only", default="", help="comma-separated op names to run")
    ap.add_argument("--cold", action="store_true",
                    help="rotating K1 batches draw fresh uniform account slots each round (cold state)")
    a = ap.parse_args()
    if a.config == "rowops":
        return rowops(a.rounds, a.out)
    if a.config == "tcn":
        return tcn(a.rounds, a.out, a.batch or 4096)
    import torch
    from igaming_platform_amd.ops import kernels as K
    from igaming_platform_amd.utils import benchkit
    from igaming_platform_amd.utils.synth import NOW0
    dev = torch.device("cuda", 0)
    S = benchkit.build(a.config, a.batch, a.accounts, dev, hot_frac=a.hot)
    sc, B = S.scorer, S.batch
    # load a request batch into the device slab once
    slot = 0
    v = sc.slab_view(slot, B)
    v[:] = S.pool[0]
    v["ts"] = NOW0
    sc._seq += 1
    sc._write_hdr(slot, B, NOW0)
    nb = 16 + 48 * B
    sc.dev_slab[:nb].copy_(sc.host_slab[slot][:nb])
    torch.cuda.synchronize()

    steps = sc.plan.steps if sc.plan else []
    tree = next((s for s in steps if s.kind == "tree"), None)
    head = next((s for s in steps if s.kind == "head"), None)
    g = sc.tree_groups.get(B, 1)
    ops = {
        "h2d_slab": lambda: sc.dev_slab[:nb].copy_(sc.host_slab[slot][:nb], non_blocking=True),
        "dedup_insert": lambda: K.dedup_insert(sc.store, sc.cfg_dev, sc.req, B, sc.hdr),
        "feature_assemble+single_update": lambda: K.feature_assemble(sc.store, sc.hdr, sc.cfg_dev, sc.req, sc.X,
                                                                     sc.feat, B, dedup=True),
        "feature_assemble_no_update": lambda: K.feature_assemble(sc.store, sc.hdr, sc.cfg_dev, sc.req, sc.X,
                                                                 sc.feat, B, dedup=False),
        "ensemble": lambda: K.ensemble(sc.hdr, sc.cfg_dev, sc.feat, sc.X, sc.ml, sc.res, B, sc.metrics),
        "update_segments": lambda: K.update_segments(sc.store, sc.cfg_dev, sc.req, B, sc.hdr),
        "d2h_results": lambda: sc.host_res[slot][:B].copy_(sc.res[:B], non_blocking=True),
    }
    if tree is not None:
        ops["tree_ensemble"] = lambda: K.tree_ensemble(tree, sc.X, None if head else sc.step_out[0], B,
                                                        partial=sc.tree_partial, groups=g, no_finish=head is not None)
    if head is not None:
        out = sc.step_out[-1]
        ops["mlp_head"] = lambda: K.mlp_head(head, sc.X, out, B, m_ptr=sc.n_ptr,
                                             tree_partial=(sc.tree_partial, g, tree) if tree else None)
    if sc.graphs:
        gc, gs, gm = sc.graphs[(B, slot)][:3]
        ops["full_step_graph"] = lambda: (gc.replay(), gs.replay(), gm.replay())
    ops_all = dict(ops)
    if a.only:
        keep = set(a.only.split(","))
        ops = {k: v for k, v in ops.items() if k in keep}
    from igaming_platform_amd.native import hipk

    def stall():  # a 300-us device spin ahead of the timed region (the Python launch path takes ~50 us)
        hipk().stall(torch.cuda.current_stream().cuda_stream, 300.0)
    times = {k: [] for k in ops}
    for r in range(a.rounds):
        # a fresh batch sequence number per round, as the scorer does per micro-batch
        sc._seq += 1
        sc._write_hdr(slot, B, NOW0)
        for k, f in ops.items():
            if k == "full_step_graph":  # the graph re-copies the slab: give it its own batch seq
                sc._seq += 1
                sc._write_hdr(slot, B, NOW0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stall()  # the device reaches e0 only after the host enqueued the op: device time only
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    # K1 phase trace of 8 sample waves (wall_clock64, 100 MHz -> us from the earliest start)
    trw = torch.zeros(((B + 15) // 16) * 4 * 16, dtype=torch.int64, device=dev)  # every wave: 16 int64
    for dd in (True, False):
        for _ in range(3):
            sc._seq += 1
            sc._write_hdr(slot, B, NOW0)
            sc.dev_slab[:nb].copy_(sc.host_slab[slot][:nb])
            if dd:
                K.dedup_insert(sc.store, sc.cfg_dev, sc.req, B, sc.hdr)
            trw.zero_()
            K.feature_assemble(sc.store, sc.hdr, sc.cfg_dev, sc.req, sc.X, sc.feat, B, dedup=dd, trace=trw)
            torch.cuda.synchronize()
        t = trw.cpu().numpy().reshape(-1, 16)[[w * 293 for w in range(7)]][:, [0, 1, 6, 7, 2, 3, 4, 5]].astype(np.float64)
        t0 = t[t > 0].min()
        print(f"K1 trace (update={dd}) us: start / level1 / live / l2-issued / level2 / compute / stores / end")
        for w in range(7):
            print("   wave", w * 293, [round((x - t0) / 100.0, 2) if x > 0 else None for x in t[w]])
    # K1 with the update on rotating pool batches (the bench's access pattern): event timing
    # of the kernel alone + phase trace of the last one
    # KB_VARIANTS: comma-separated masks (512 = also store the D2H feature images into pinned host
    # memory, as the serving path does; 1024 = a second launch right behind the first)
    fenc_host = torch.zeros((B, 32), dtype=torch.int32).pin_memory()
    modes = [(v, 0) for v in os.environ.get("KB_K1_MODES", "full").split(",") if v not in ("", "-")]
    modes += [("full", int(m)) for m in os.environ.get("KB_VARIANTS", "").split(",") if m]
    for var, abl in modes:  # full | nodedup | noseg
      ts_k1 = []
      for i in range(24):
          vv = sc.slab_view(slot, B)
          vv[:] = S.pool[i % len(S.pool)]
          if a.cold:  # every round a fresh uniform draw over the population: cold account lines
              vv["slot"] = np.random.default_rng(1000 + i).integers(0, a.accounts, B).astype(np.int32)
          vv["ts"] = NOW0 + 1 + i
          sc._seq += 1
          sc._write_hdr(slot, B, NOW0 + 1 + i)
          sc.dev_slab[:nb].copy_(sc.host_slab[slot][:nb])
          if var != "nodedup":
              K.dedup_insert(sc.store, sc.cfg_dev, sc.req, B, sc.hdr)
          trw.zero_()
          e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
          stall()
          e0.record()
          K.feature_assemble(sc.store, sc.hdr, sc.cfg_dev, sc.req, sc.X, sc.feat, B, dedup=var != "nodedup", trace=trw,
                             fenc=fenc_host if abl & 512 else None)
          if abl & 1024:  # the same launch again right behind it (instruction caches warm): 2 launches timed
              K.feature_assemble(sc.store, sc.hdr, sc.cfg_dev, sc.req, sc.X, sc.feat, B, dedup=False,
                                 fenc=fenc_host if abl & 512 else None)
          e1.record()
          e1.synchronize()
          ts_k1.append(e0.elapsed_time(e1) * 1e3)
          if var not in ("nodedup", "noseg"):
              K.update_segments(sc.store, sc.cfg_dev, sc.req, B, sc.hdr)
      full = trw.cpu().numpy().reshape(-1, 16)
      if os.environ.get("KB_TRACE_OUT"):
          np.save(os.environ["KB_TRACE_OUT"] + f"_a{abl}.npy", full)
      print(f"[{var} variant={abl}] K1+update on rotating pool batches: median {np.median(ts_k1[8:]):.1f} us "
            f"(first pass {np.median(ts_k1[:8]):.1f})")
      t = full[[w * 293 for w in range(7)]][:, [0, 1, 6, 7, 2, 3, 4, 5]].astype(np.float64)
      t0 = t[t > 0].min()
      print("K1 trace (update, rotating batches) us: start / level1 / live / l2-issued / level2 / compute / stores / end")
      for w in range(7):
          print("   wave", w * 293, [round((x - t0) / 100.0, 2) if x > 0 else None for x in t[w]])
    # mlp_head (8 sample blocks) phase trace
    tr = torch.zeros(64, dtype=torch.int64, device=dev)
    if head is not None:
        for _ in range(3):
            tr.zero_()
            ops["mlp_head"]() if "mlp_head" in ops else None
            K.mlp_head(head, sc.X, sc.step_out[-1], B, m_ptr=sc.n_ptr,
                       tree_partial=(sc.tree_partial, g, tree) if tree else None, trace=tr)
            torch.cuda.synchronize()
        t = tr.cpu().numpy().reshape(8, 8)[:, :5].astype(np.float64)
        if (t > 0).any():
            t0 = t[t > 0].min()
            print("mlp_head trace us: start / staged / mfma done / synced / stored")
            for b in range(8):
                print("   block", b * 32, [round((x - t0) / 100.0, 2) if x > 0 else None for x in t[b]])
    res = {k: dict(median_us=float(np.median(v[min(5, len(v) - 1):])), min_us=float(np.min(v[min(5, len(v) - 1):])))
           for k, v in times.items()}
    for k, v in res.items():
        print(f"{k:28s} median {v['median_us']:8.1f} us   min {v['min_us']:8.1f} us")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(config=a.config, batch=B, kernels=res), f, indent=1)


if __name__ == "__main__":
    main()
