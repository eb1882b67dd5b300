#!/usr/bin/env python3
"""K22, mesh -> signed distance, timed by HIP events (medians of --reps runs after a warm-up; every workload's spread against
itself is printed as min .. max):
  g9 65^3        : tests/golden/g9_mesh.npz (32 970 faces) on its own 65^3 grid, band 3 and band inf
  config 3 256^3 : the marching-cubes mesh of the config-3 scene (256^3, 3 views of camera C2) back onto the 256^3 grid, band 4
  points         : 100 000 points against the same mesh: scattered through the config-3 volume at band inf and band 4, and within
                   ~2 voxels of the surface at band inf (query() hands them to the kernel in Morton order of their cells)
  evaluation rate: a 1 280-face icosphere in ONE cell (cell larger than the mesh) on a 65^3 grid, band inf: there every lane
                   evaluates every face exactly once, so point-face evaluations = waves * 64 * faces is known without a counter
and the host cost of building a MeshDistance (pseudonormal tables in numpy, the plan, the upload and the table build).
--parent-lib PATH: config 3's table build (dfh_mesh_sdf_build) and the 256^3 grid behind it through this build's library and
through the parent commit's (tools/parent_lib.py): cell starts, the .dist grid, closest points and faces compared bit for bit, then
both timed, alternating, two rounds each.
usage: python tools/kbench_mesh_sdf.py [--reps 10] [--no-256] [--parent-lib build_variants/parent.so] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamicfusion_body_amd import FusionDM, mesh, scene

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-256", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=None):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps or a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def host_cost(name, v, f):
    t0 = time.perf_counter()
    mesh.pseudonormals(v, f)
    t1 = time.perf_counter()
    md = mesh.MeshDistance(v, f)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    lay = md.layout
    say("%s: %d vertices, %d faces; tables (numpy) %.1f ms; MeshDistance() in all %.1f ms; cell %.3g, table %s cells, %d entries, %.1f MB"
        % (name, len(v), len(f), 1e3 * (t1 - t0), 1e3 * (t2 - t1), lay.cell, "x".join(str(d) for d in lay.dims), lay.n_entries,
           lay.bytes / 2 ** 20))
    return md


def config3_mesh(R=256):
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    fdm = FusionDM(tdist, K, tsdf_res=R)
    T, Wt = fdm._new_volume_pair()
    for ang in (0.0, 40.0, -40.0):
        lw = scene.view_extrinsic(ang)
        dm = scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)
        fdm.fuseDepths(torch.from_numpy(dm).cuda(), lw, T, Wt, scale=scale, center=center)
    v, f, _, _ = mesh.marching_cubes(T, 0.0, as_numpy=True)
    return v, f


say("K22 mesh -> signed distance on %s, %d reps" % (torch.cuda.get_device_name(0), a.reps))
d = np.load(os.path.join(ROOT, "tests", "golden", "g9_mesh.npz"))
md = host_cost("g9", d["verts"], d["faces"])
out = torch.empty((65, 65, 65), dtype=torch.float32, device="cuda")
for band in (3.0, math.inf):
    say("g9 65^3 band %-4g: %8.3f ms  (%.3f .. %.3f)" % ((band,) + timed(lambda: md.grid(0.0, 1.0, (65, 65, 65), band, out=out))))

if not a.no_256:
    v, f = config3_mesh()
    md3 = host_cost("config 3", v, f)
    out = torch.empty((256, 256, 256), dtype=torch.float32, device="cuda")
    say("config 3 256^3 band 4: %8.3f ms  (%.3f .. %.3f)" % timed(lambda: md3.grid(0.0, 1.0, (256, 256, 256), 4.0, out=out), max(3, a.reps // 2)))
    P = torch.from_numpy(np.random.RandomState(0).uniform(0, 255, (100000, 3))).cuda()
    say("100k points, band inf : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: md3.query(P), max(3, a.reps // 2)))
    say("100k points, band 4   : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: md3.query(P, 4.0)))
    near = torch.from_numpy(v[np.random.RandomState(1).randint(0, len(v), 100000)] + np.random.RandomState(2).normal(0, 2.0, (100000, 3))).cuda()
    say("100k points within ~2 voxels of the surface, band inf: %8.3f ms  (%.3f .. %.3f)" % timed(lambda: md3.query(near)))
    if a.parent_lib:
        import parent_lib
        from dynamicfusion_body_amd import _lib
        from dynamicfusion_body_amd.device import current_stream_ptr
        n_cells = int(np.prod(list(md3.layout.dims)))

        def build(lib):
            _lib.check(lib.dfh_mesh_sdf_build(md3._m, current_stream_ptr()), "dfh_mesh_sdf_build")
            return (md3._table.view(torch.int32)[:n_cells + 1],)

        def build_and_grid(lib):
            md3.lib = lib
            return build(lib) + tuple(md3.grid(0.0, 1.0, (256, 256, 256), 4.0, out=out, want_closest=True, want_face=True))
        names = ["dfh_mesh_sdf_build", "dfh_mesh_sdf_grid"]
        parent_lib.against_parent(say, "config 3 table build, %d cells" % n_cells, build, names, a.parent_lib, a.reps)
        parent_lib.against_parent(say, "config 3 table build + 256^3 grid", build_and_grid, names, a.parent_lib, max(3, a.reps // 2))

sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_sdf_cases as MC
sv, sf = MC.icosphere(3, 20.0, 32.0)
one = mesh.MeshDistance(sv, sf, cell=1000.0)
out = torch.empty((65, 65, 65), dtype=torch.float32, device="cuda")
ms, lo, hi = timed(lambda: one.grid(0.0, 1.0, (65, 65, 65), math.inf, out=out))
evals = 17 ** 3 * 64 * len(sf)
say("evaluation rate: %d faces in one cell, 65^3 grid: %.3f ms (%.3f .. %.3f), %.3g point-face evaluations, %.3g per second"
    % (len(sf), ms, lo, hi, evals, evals / (ms * 1e-3)))
if a.out:
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")
