#!/usr/bin/env python3
"""dfh_nearest_descriptors (K14), the exact kernel against the fast path (profiles/r14_descriptors.txt).

Inputs: the fused scene at --res (the 8-view orbit of the benchmark's camera, as config 3 / config 5 build it), its mesh at
marching-cubes step 3 (the canonical mesh: queries) against its mesh at step 1 (the live mesh: base); descriptors of --dim
channels = a fixed random linear map of the vertex position plus unit normal noise, float32.  HIP events around the call, warm,
the two paths alternating and each timed TWICE per round (A B A' B'), medians of --runs: the spread between a path's twins is the
noise a difference has to exceed.  Reported: both paths, stats_out, the share of the 157 TFLOP/s float32 matrix peak at
2 Q L D flops, what dfh_nearest_descriptors_path picks, and (--host) scipy's cKDTree on the same arrays for scale."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamicfusion_body_amd import _lib, kernels, mesh, scene
from dynamicfusion_body_amd.device import current_stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--res", default="256,512")
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--host", action="store_true", help="also time scipy's cKDTree (minutes at 512^3)")
ap.add_argument("--host-queries", type=int, default=2000, help="queries of the host run (scaled to all of them in the report)")
ap.add_argument("--small", action="store_true", help="also a ladder of small random problems, for the size threshold of the default")
a = ap.parse_args()
PEAK = 157e12


def meshes(R):
    H, W, fx, cx, cy = scene.CAMERAS["C2" if R <= 256 else "C5"]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    T = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    Wt = torch.zeros((R, R, R), dtype=torch.float32, device="cuda")
    for v in range(8):
        lw = scene.view_extrinsic(45.0 * v)
        d = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
        kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist)
    canon = mesh.marching_cubes(T, 0.0, 3)[0]
    live = mesh.marching_cubes(T, 0.0, 1)[0]
    del T, Wt
    torch.cuda.empty_cache()
    return canon, live


def call(lib, q, b, idx, d2, stats, ws):
    _lib.check(lib.dfh_nearest_descriptors(q.data_ptr(), q.shape[0], b.data_ptr(), b.shape[0], q.shape[1], idx.data_ptr(), d2.data_ptr(),
                                           stats.data_ptr(), ws.data_ptr(), ws.numel(), current_stream_ptr()), "dfh_nearest_descriptors")


def timed(lib, path, *args):
    _lib.set_option("nd_path", path)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(lib, *args)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(name, q, b, runs, host):
    lib = _lib.load()
    nq, nb, dim = q.shape[0], b.shape[0], q.shape[1]
    idx = torch.empty(nq, dtype=torch.int32, device="cuda")
    d2 = torch.empty(nq, dtype=torch.float64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(16, lib.dfh_nearest_descriptors_workspace_bytes(nq, nb, dim)), dtype=torch.uint8, device="cuda")
    args = (q, b, idx, d2, stats, ws)
    out = {}
    for path in (1, 2):                                              # warm-up, and the two results
        timed(lib, path, *args)
        out[path] = (idx.clone(), d2.clone(), stats.cpu().tolist())
    same = torch.equal(out[1][0], out[2][0]) and torch.equal(out[1][1].view(torch.int64), out[2][1].view(torch.int64))
    t = {(1, 0): [], (2, 0): [], (1, 1): [], (2, 1): []}
    for _ in range(runs):
        for twin in (0, 1):
            for path in (1, 2):
                t[(path, twin)].append(timed(lib, path, *args))
    med = {k: statistics.median(v) for k, v in t.items()}
    _lib.set_option("nd_path", None)
    picked = lib.dfh_nearest_descriptors_path(nq, nb, dim)
    flops = 2.0 * nq * nb * dim
    spread = max(abs(med[(1, 0)] - med[(1, 1)]), abs(med[(2, 0)] - med[(2, 1)]))
    fast = 0.5 * (med[(2, 0)] + med[(2, 1)])
    exact = 0.5 * (med[(1, 0)] + med[(1, 1)])
    print("%-10s Q=%7d L=%7d D=%d | exact %9.3f / %9.3f ms | fast %9.3f / %9.3f ms (twins, medians of %d; twin spread %.3f ms) | "
          "exact/fast %.2fx | fast: %.1f%% of the f32 matrix peak at 2QLD | stats %s (%.2f pairs per query) | library picks path %d | "
          "same bits: %s" % (name, nq, nb, dim, med[(1, 0)], med[(1, 1)], med[(2, 0)], med[(2, 1)], runs, spread, exact / fast,
                             100.0 * flops / (fast * 1e-3) / PEAK, out[2][2], out[2][2][0] / max(nq, 1), picked, same), flush=True)
    if host:
        from scipy.spatial import cKDTree
        qh, bh = q.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(bh)
        t1 = time.perf_counter()
        m = min(a.host_queries, nq)
        _, ref = tree.query(qh[:m])
        t2 = time.perf_counter()
        agree = float((ref == out[1][0][:m].cpu().numpy()).mean())
        print("%-10s host cKDTree: build %.1f ms, %d queries %.1f ms -> %.0f ms for all %d (one thread); agreement with the device %.4f"
              % (name, (t1 - t0) * 1e3, m, (t2 - t1) * 1e3, (t2 - t1) * 1e3 * nq / m, nq, agree), flush=True)


torch.manual_seed(14)
M = torch.randn(3, a.dim, dtype=torch.float64, device="cuda")
for R in [int(x) for x in a.res.split(",") if x]:
    canon, live = meshes(R)
    feats = lambda v: (v.to(torch.float64) @ M + torch.randn(v.shape[0], a.dim, dtype=torch.float64, device="cuda")).to(torch.float32).contiguous()
    measure("%d^3" % R, feats(canon), feats(live), a.runs, a.host)
if a.small:
    for n in (64, 128, 256, 1024, 2048, 4096, 16384):
        q = torch.randn(n, a.dim, device="cuda")
        b = torch.randn(n, a.dim, device="cuda")
        measure("random", q, b, a.runs, False)
