#!/usr/bin/env python3
"""K25, mesh smoothing (Taubin's lambda|mu filter over a fixed Laplacian) and vertex normals, timed by HIP events (medians of
--reps runs after a warm-up run; each line's spread against itself is printed as min .. max) on
  config 3 : the marching-cubes mesh of the config-3 scene (256^3, 3 views of camera C2)
  config 5 : the marching-cubes mesh of the config-5 scene (512^3, the 8-view orbit of camera C5)
per mesh: the stable torch.sort of the corner entries, prepare in both weight modes (it synchronises, so the events bracket a
host wait too), one pass in each weight mode and each value layout (a 10-pass call minus a 0-pass call, over 10: the widening
and the final rounding are in both), the pass's byte floor and the rate and share of the 8.0 TB/s HBM peak that gives, a
10-iteration Taubin call, vertex_normals, an unordered torch.index_add_ formulation of one uniform pass (not bit-reproducible:
float atomics), and beside them marching_cubes, filter_components and simplify on the same mesh in the same run.
usage: python tools/kbench_smooth.py [--reps 20] [--no-512] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamicfusion_body_amd import FusionDM, mesh, scene
from dynamicfusion_body_amd.pipeline import SlabFrame

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-512", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []
HBM_PEAK = 8.0e12


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def config3_volume(R=256):                                  # (the two scene volumes of kbench_simplify.py)
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    fdm = FusionDM(tdist, K, tsdf_res=R)
    T, Wt = fdm._new_volume_pair()
    for ang in (0.0, 40.0, -40.0):
        lw = scene.view_extrinsic(ang)
        dm = scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)
        fdm.fuseDepths(torch.from_numpy(dm).cuda(), lw, T, Wt, scale=scale, center=center)
    return T


def config5_volume(R=512):
    H, W, fx, cx, cy = scene.CAMERAS["C5"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, None, None, knn=4, pcg_iters=10, band=4.0, distributed=False)
    for v in range(8):
        lw = scene.view_extrinsic(45.0 * v)
        sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda(), lw)
    return sf.T


def pass_floor_bytes(V, F, weights):
    """What one pass must move at the least: the neighbour pairs (8 B an entry) and the list bounds (8 B a vertex), the weight
    pairs (16 B an entry, cotangent only), every position row gathered once (24 B) and one store (24 B), the flag (1 B)."""
    return 3 * F * 8 + V * 8 + (3 * F * 16 if weights == "cotangent" else 0) + V * 24 + V * 24 + V


def index_add_pass(x, f, lam):
    """One uniform pass with float atomics: every face adds its two differences to each of its three corners."""
    acc = torch.zeros_like(x)
    cnt = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    two = torch.full((f.shape[0],), 2.0, dtype=x.dtype, device=x.device)
    for c in range(3):
        v, p, q = f[:, c].long(), f[:, (c + 1) % 3].long(), f[:, (c + 2) % 3].long()
        acc.index_add_(0, v, (x[p] - x[v]) + (x[q] - x[v]))
        cnt.index_add_(0, v, two)
    return x + lam * torch.where(cnt[:, None] > 0, acc / cnt[:, None], torch.zeros_like(acc))


def measure(name, T, level):
    mc = lambda: mesh.marching_cubes(T, level)
    v, f, nrm, _ = mc()
    V, F = v.shape[0], f.shape[0]
    say("%s: %d vertices, %d faces" % (name, V, F))
    say("  marching_cubes (same volume)         : %8.3f ms  (%.3f .. %.3f)" % timed(mc))
    say("  filter_components(min_faces=10)      : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.filter_components(v, f, nrm, min_faces=10)))
    say("  simplify(cell=2, quadric)            : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.simplify(v, f, nrm, cell=2.0)))
    say("  torch.sort of the 3F corner entries  : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: torch.sort(f.reshape(-1), stable=True)))
    for weights in ("uniform", "cotangent"):
        say("  MeshLaplacian(%-9s) sort+prepare : %8.3f ms  (%.3f .. %.3f)" % ((weights,) + timed(lambda: mesh.MeshLaplacian(v, f, weights))))
        L = mesh.MeshLaplacian(v, f, weights)
        say("    flagged vertices: %d" % int(L.boundary.sum()))
        results = {}
        for layout in ("rows", "planes"):
            L.layout = layout
            t0 = timed(lambda: L.smooth(iters=0))
            t10 = timed(lambda: L.smooth(iters=10, mu=0.0))
            per = (t10[0] - t0[0]) / 10.0
            floor = pass_floor_bytes(V, F, weights)
            rate = floor / (per * 1e-3)
            say("    %-6s: 0-pass call %7.3f ms (%.3f .. %.3f), 10-pass call %7.3f ms (%.3f .. %.3f) -> one pass %7.4f ms; floor %.1f MB -> %.2f TB/s, %.0f %% of "
                "the 8.0 TB/s peak" % (layout, *t0, *t10, per, floor / 1e6, rate / 1e12, 100.0 * rate / HBM_PEAK))
            say("    %-6s: 10 Taubin iterations (20 passes)   : %8.3f ms  (%.3f .. %.3f)" % ((layout,) + timed(lambda: L.smooth(iters=10))))
            results[layout] = L.smooth(iters=10)
        say("    rows and planes give the same bits: %s" % torch.equal(results["rows"], results["planes"]))
        L.layout = "rows"
        say("    attribute of width 1, 10 Taubin iterations : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: L.smooth(nrm[:, 0].contiguous(), iters=10)))
        say("    vertex_normals                             : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: L.vertex_normals(sign=-1.0)))
    x = v.double()
    say("  one uniform pass by torch.index_add_ (fp64, unordered float atomics): %8.3f ms  (%.3f .. %.3f)" % timed(lambda: index_add_pass(x, f, 0.5)))
    free = mesh.MeshLaplacian(v, f, "uniform", "free")
    d = (index_add_pass(x, f, 0.5) - free.smooth(x, iters=1, mu=0.0)).abs().max()
    say("    max |index_add_ - kernel| after one pass (boundary free): %.3g" % float(d))
    say("  smooth_with_normals(iters=10), the hook's whole call : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.smooth_with_normals(v, f, 10)))


say("K25 mesh smoothing on %s, %d reps" % (torch.cuda.get_device_name(0), a.reps))
T3 = config3_volume()
measure("config 3 (256^3)", T3, 0.0)
del T3
torch.cuda.empty_cache()
if not a.no_512:
    measure("config 5 (512^3)", config5_volume(), 0.0)
if a.out:
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")
