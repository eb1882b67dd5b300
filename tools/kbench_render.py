#!/usr/bin/env python3
"""Per-stage times of rendering the live model at config 5's size (HIP events): the 512^3 canonical sphere (an analytic SDF,
truncated at 4 voxels), 2 048 Fibonacci nodes with small translations, 8 views of 1280x720.  Stages: marching cubes (level 0,
reference order), knn of every vertex (sample_knn), warp (warp_points), raster (dfh_render_raster: key clear + the two raster
launches), resolve (dfh_render_resolve, normals on).  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dynamicfusion_body_amd import mesh, scene, solve  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=512)
ap.add_argument("--nodes", type=int, default=2048)
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()

R = a.res
H, W, fx, cx, cy = scene.CAMERAS["C5"]
K = scene.intrinsics(fx, cx, cy)
scale, center, tdist = scene.grid_params(R)
rv = scene.SPHERE_R / scale
g = torch.arange(R, dtype=torch.float32, device="cuda") - R / 2
T = torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) - rv
T.clamp_(-tdist / scale, tdist / scale)
T = T.contiguous()
node_pos, node_w = scene.fibonacci_nodes(a.nodes, R)
rng = np.random.default_rng(0)
node_dq = np.zeros((a.nodes, 8))
node_dq[:, 0] = 1.0
node_dq[:, 5:8] = 0.5 * rng.uniform(-0.5, 0.5, (a.nodes, 3))
P, Q, Wn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (node_pos, node_dq, node_w))
ident = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
lws = [scene.view_extrinsic(45.0 * v) for v in range(a.views)]

times = {}


def run(record):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    ev[0].record()
    v, f, n, _ = mesh.marching_cubes(T, 0.0, 1)
    ev[1].record()
    nbr, _ = solve.sample_knn(v, P, Wn, 4)
    ev[2].record()
    vp, vn = solve.warp_points(v, n, ident, nbr=nbr, node_dq=Q, node_pos=P, node_w=Wn)
    ev[3].record()
    k = [4]

    def stage(name):
        ev[k[0]].record()
        k[0] += 1
    depth, normal, face = mesh.render(vp, f, vn, K, lws, H, W, scale=scale, center=center, half=R / 2, stages=stage)
    torch.cuda.synchronize()
    if record:
        for i, name in enumerate(("mc", "knn", "warp", "raster", "resolve")):
            times.setdefault(name, []).append(ev[i].elapsed_time(ev[i + 1]))
    return v.shape[0], f.shape[0], depth


for _ in range(2):
    run(False)
for _ in range(a.reps):
    nv, nf, depth = run(True)
covered = int((depth != 0).sum())
res = {"tool": "kbench_render", "res": R, "nodes": a.nodes, "views": a.views, "H": H, "W": W, "vertices": nv, "faces": nf,
       "pixels_covered": covered, "ms_median": {k: float(np.median(v)) for k, v in times.items()},
       "ms_min": {k: float(np.min(v)) for k, v in times.items()}, "reps": a.reps}
res["ms_median"]["total"] = float(sum(res["ms_median"].values()))
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write(line + "\n")
