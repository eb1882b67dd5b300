#!/usr/bin/env python3
"""K15: the vertex-id pass (dfh_render_raster + dfh_render_vertex_ids) and the pooling call (dfh_pool_features) on the
reference's own workload (profiles/r15_pool.txt): 24 views of 512 x 512, 16 channels.

Inputs: the fused scene at --res (the 8-view orbit of the benchmark's camera, as tools/kbench_descriptors.py builds it), its
mesh at marching-cubes step 1, regularised and rendered from descriptors.turntable_views(); features = a fixed pseudo-random
float32 tensor (V, H, W, D).  HIP events around the calls, warm, medians of --runs, every figure TWICE (twins: the spread between
them is the noise a difference has to exceed).  Reported: the id pass (both 16-view batches); the pooling call, its bytes
(below) and the rate they make; torch.index_add_ on the same data for scale (an UNORDERED atomic sum: not the same bits, and it
still lacks the count and the division); the host loop of the restatement (tests/pool_np.py, on --host-pixels pixels, scaled).

Bytes of the pooling call, counted from its passes (n pixels, c of them covered, m vertices, D channels, 4-byte words):
vid twice (count, scatter) 8 n; the counts and offsets as the passes read and write them 24 m; the slots written and read
8 c; the pixel list written, ordered (read + written) and read 16 c; the covered feature rows 4 D c; the result 4 D m.
--parent-lib PATH: the pooling call through this build's library and through the parent commit's (tools/parent_lib.py): features and
counts compared bit for bit, then both timed, alternating, two rounds each."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from dynamicfusion_body_amd import _lib, descriptors, kernels, mesh, scene

ap = argparse.ArgumentParser()
ap.add_argument("--res", default="256,512")
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--host-pixels", type=int, default=200000, help="pixels of the host loop (0: skip it)")
ap.add_argument("--copy-gbs", type=float, default=0.0, help="the copy ceiling bench.py's micro-benchmark reports, for the share")
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()


def scene_mesh(R):
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
    verts, faces = mesh.marching_cubes(T, 0.0, 1)[:2]
    del T, Wt
    torch.cuda.empty_cache()
    return verts, faces


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def twins(fns, runs):
    """{name: (median of twin 0, median of twin 1)} with the candidates alternating, A B A' B'."""
    t = {(n, k): [] for n in fns for k in (0, 1)}
    for n in fns:
        timed(fns[n])                                                # warm
    for _ in range(runs):
        for k in (0, 1):
            for n in fns:
                t[(n, k)].append(timed(fns[n])[0])
    return {n: (statistics.median(t[(n, 0)]), statistics.median(t[(n, 1)])) for n in fns}


def measure(R):
    lib = _lib.load()
    verts, faces = scene_mesh(R)
    reg = torch.from_numpy(descriptors.regularize_mesh(verts.cpu().numpy())).cuda()
    n_verts, S, D = reg.shape[0], a.size, a.dim
    K, lws = descriptors.turntable_views(width=S, height=S)
    ws = mesh.render_workspace(16, S, S, faces.shape[0])
    ids = lambda: mesh.render_vertex_ids(reg, faces, K, lws, S, S, 1.0, 3.5, workspace=ws)
    vid, image = ids()
    g = torch.Generator(device="cuda").manual_seed(15)
    feats = torch.randn((len(lws), S, S, D), generator=g, device="cuda", dtype=torch.float32)
    n = vid.numel()
    covered = int((vid >= 0).sum())
    pool = lambda: descriptors.pool_features(vid, feats, n_verts)
    feat, cnt = pool()
    flat_vid, flat_feats = vid.reshape(-1), feats.reshape(n, D)
    sel = torch.nonzero(flat_vid >= 0).reshape(-1)
    sel_vid = flat_vid[sel].to(torch.int64)

    def index_add():
        acc = torch.zeros((n_verts, D), dtype=torch.float32, device="cuda")
        return acc.index_add_(0, sel_vid, flat_feats[sel])
    res = twins({"ids": ids, "pool": pool, "index_add": index_add}, a.runs)
    again = pool()
    same = torch.equal(again[0].view(torch.int32), feat.view(torch.int32)) and torch.equal(again[1], cnt)
    c = cnt.to(torch.int64)
    nbytes = 8 * n + 24 * n_verts + 24 * covered + 4 * D * covered + 4 * D * n_verts
    ms = 0.5 * sum(res["pool"])
    rate = nbytes / (ms * 1e-3) / 1e9
    share = " = %.1f%% of the %.0f GB/s copy ceiling" % (100.0 * rate / a.copy_gbs, a.copy_gbs) if a.copy_gbs > 0 else ""
    print("%d^3: %d vertices, %d faces | %d views of %dx%d, D=%d | covered %d of %d pixels (%.1f%%), vertices seen %.1f%%, pixels per seen "
          "vertex median %d max %d | id pass %.3f / %.3f ms | pool %.3f / %.3f ms (%.1f MB, %.0f GB/s%s) | torch.index_add_ (unordered, "
          "gather included) %.3f / %.3f ms | twins, medians of %d | two pooling runs bit-identical: %s"
          % (R, n_verts, faces.shape[0], len(lws), S, S, D, covered, n, 100.0 * covered / n, 100.0 * float((c > 0).float().mean()),
             int(c[c > 0].median()), int(c.max()), *res["ids"], *res["pool"], nbytes / 1e6, rate, share, *res["index_add"], a.runs, same),
          flush=True)
    if a.parent_lib:
        import parent_lib
        parent_lib.against_parent(print, "%d^3: pool_features" % R, lambda lib: pool(), ["dfh_pool_features"], a.parent_lib, a.runs)
    if a.host_pixels > 0:
        import pool_np as PN
        hv = flat_vid[sel[:a.host_pixels]].cpu().numpy()
        hf = flat_feats[sel[:a.host_pixels]].cpu().numpy()
        t0 = time.perf_counter()
        PN.pool_features_loop(hv[:0], hf[:0], n_verts)               # the per-vertex part alone: not scaled with the pixels
        t1 = time.perf_counter()
        PN.pool_features_loop(hv, hf, n_verts)
        t2 = time.perf_counter()
        per_vertex, per_pixel = t1 - t0, (t2 - t1) - (t1 - t0)
        print("%d^3: host loop of the restatement: %d covered pixels %.2f s, the %d vertices %.2f s -> %.1f s for all %d pixels (one thread)"
              % (R, len(hv), per_pixel, n_verts, per_vertex, per_pixel * covered / max(len(hv), 1) + per_vertex, covered), flush=True)


for R in [int(x) for x in a.res.split(",") if x]:
    measure(R)
