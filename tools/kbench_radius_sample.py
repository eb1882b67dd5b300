#!/usr/bin/env python3
"""Radius subsampling, host loop against device rounds (profiles/r10_radius_sample.txt).

Inputs: the |d| < 1 shells of a sphere in a 64^3 / 128^3 / 256^3 grid (voxel centres, x-major; radius 6 / 8 / 12) and the
config-5 sample set (512^3, the 8-view orbit, band 4: the frame loop's band samples in canonical order; radius = the mean node
spacing of 2 048 nodes).  Per input: graph.uniform_sample on the host (wall time) and dfh_radius_sample on the device (HIP
events around the call, and wall time), host and device alternating, each the median of --runs runs; the index lists are
compared.  --host-runs-c5 bounds the host runs of the config-5 set (minutes each); 0 skips them.
--parent-lib PATH: every input also through the parent commit's library (tools/parent_lib.py): count and indices compared, then both
libraries timed, alternating, two rounds each."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamicfusion_body_amd import _lib, graph, scene
from dynamicfusion_body_amd.pipeline import SlabFrame

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=10)
ap.add_argument("--host-runs-c5", type=int, default=1)
ap.add_argument("--no-c5", action="store_true")
ap.add_argument("--shells", default="64,128,256")
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()


def shell(res):
    r = {64: 20.0, 128: 40.0, 256: 75.0}[res]
    ax = torch.arange(res, dtype=torch.float64, device="cuda")
    g = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    d = (g - (res - 1) / 2.0).norm(dim=1) - r
    return g[d.abs() < 1.0].contiguous()


def config5():
    R = 512
    H, W, fx, cx, cy = scene.CAMERAS["C5"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, None, None, knn=4, pcg_iters=10, band=4.0, distributed=False)
    for v in range(8):
        lw = scene.view_extrinsic(45.0 * v)
        sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda(), lw)
    pts, _ = sf.band_samples()
    pts = SlabFrame._canonical_order(pts).contiguous()
    _, node_w = scene.fibonacci_nodes(2048, R)
    del sf
    torch.cuda.empty_cache()
    return pts, 0.5 * float(node_w[0])


def device_run(lib, P, radius, ws, idx):
    count, rounds = ctypes.c_long(0), ctypes.c_int(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    _lib.check(lib.dfh_radius_sample(P.data_ptr(), P.shape[0], radius, idx.data_ptr(), idx.numel(), ctypes.byref(count),
                                     ctypes.byref(rounds), ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream().cuda_stream),
               "dfh_radius_sample")
    e1.record()
    wall = (time.perf_counter() - t0) * 1e3                 # (the call has synchronised the stream when it returns)
    e1.synchronize()
    return e0.elapsed_time(e1), wall, count.value, rounds.value


def measure(name, P, radius, runs, host_runs):
    lib = _lib.load()
    n = P.shape[0]
    ws = torch.empty((lib.dfh_radius_sample_workspace_bytes(n) + 7) // 8, dtype=torch.int64, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    host_pts = P.cpu().numpy()
    device_run(lib, P, radius, ws, idx)                     # warm-up (code objects, the pinned counter words)
    ev, wall, host, want = [], [], [], None
    for r in range(runs):
        if r < host_runs:
            t0 = time.perf_counter()
            _, want = graph.uniform_sample(host_pts, radius)
            host.append((time.perf_counter() - t0) * 1e3)
        e, w, count, rounds = device_run(lib, P, radius, ws, idx)
        ev.append(e); wall.append(w)
    same = "not compared" if want is None else str(bool(np.array_equal(idx[:count].cpu().numpy(), np.asarray(want))))
    med = statistics.median
    print("%-12s n=%8d radius=%6.2f nodes=%5d rounds=%4d | device %9.3f ms (events) %9.3f ms (wall), median of %d | host %s | same indices: %s"
          % (name, n, radius, count, rounds, med(ev), med(wall), runs,
             "%10.1f ms, median of %d" % (med(host), len(host)) if host else "not run", same), flush=True)
    if a.parent_lib:
        import parent_lib

        def call(through):
            count = device_run(through, P, radius, ws, idx)[2]
            return idx[:count], torch.tensor([count])
        parent_lib.against_parent(print, name, call, ["dfh_radius_sample"], a.parent_lib, runs)


for res in [int(x) for x in a.shells.split(",") if x]:
    measure("shell %d^3" % res, shell(res), {64: 6.0, 128: 8.0, 256: 12.0}[res], a.runs, a.runs)
if not a.no_c5:
    P, radius = config5()
    measure("config 5", P, radius, a.runs, a.host_runs_c5)
