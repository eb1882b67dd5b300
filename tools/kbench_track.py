#!/usr/bin/env python3
"""K21, camera tracking, timed by HIP events (medians, each figure timed twice so that its spread against itself is on record):
per pyramid level one ICP iteration (the slope between a 1- and a 9-iteration call of kernels.icp_track: two launches each), the
halving and the level's normal map, and CameraTracker.track as a whole -- at 640 x 480 with 1 view and at 1280 x 720 with 8 views
of the bench scene, the model a 256^3 volume fused from the same cameras and ray-cast per level.  Beside each iteration its byte
floor (32 B per live pixel: live and model depth and normals, read once) and the step of dfh_gn_global_sampled at config 3
(256^3, 512 nodes, 3 views, every 4th tile), the nearest sibling.
usage: python tools/kbench_track.py [--reps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamicfusion_body_amd import kernels, scene, tracking
from dynamicfusion_body_amd.pipeline import SlabFrame

HBM_TBS = 8.0                                  # nominal peak, for the byte floor only
CASES = [("C2", (0.0,)), ("C5", tuple(45.0 * v for v in range(8)))]
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(variants, reps):
    """name -> (median of round 0, median of round 1, min) in us; the variants alternate."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name in variants for rnd in (0, 1)}
    for rep in range(reps + 2):
        for rnd in (0, 1):
            for name, fn in variants.items():
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    return {name: (statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)]), min(times[(name, 0)] + times[(name, 1)]))
            for name in variants}


def track_case(cam, angles):
    R = 256
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(x) for x in angles]
    V = len(lws)
    model_depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]
    off = np.array([0.4, -0.25, 0.15]) * scale
    live = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda() for lw in lws]
    T = torch.empty((R, R, R), dtype=torch.float32, device="cuda")
    Wt = torch.empty_like(T)
    kernels.integrate_depth_views(T, Wt, model_depths, K, np.linalg.inv(K), lws, scale, center, tdist, fresh=tdist / scale)
    tr = tracking.CameraTracker(K, 3, (4, 5, 10), (2 * scale, 4 * scale, 8 * scale), (0.8, 0.65, 0.5), max_jump=4 * scale)
    maps = {}

    def model(lw, Kl, h, w):
        if (h, w) not in maps:
            r = kernels.raycast(T, Wt, Kl, np.linalg.inv(Kl), lw, h, w, scale, center)
            maps[(h, w)] = (r.depth, r.normals)
        return maps[(h, w)]
    lws1, stats = tr.track(live, lws, model)
    say("%s: %d view(s) of %dx%d; model: 256^3 ray-cast per level; live: the sphere moved by (0.4, -0.25, 0.15) voxels" % (cam, V, W, H))
    say("  track(): lost %s; rows at the finest level %s; statuses per level (finest first) %s"
        % (stats["lost"].tolist(), stats["levels"][0][:, -1, 28].astype(int).tolist(),
           [int(s[:, :, 29].sum()) for s in stats["levels"]]))
    pyr = tr.live_pyramid(live)
    scratch = kernels.icp_track_scratch(V)
    Tid = torch.eye(4, dtype=torch.float64)[:3].repeat(V, 1, 1).cuda().contiguous()
    variants = {}
    for l in range(3):
        d, n = pyr[l]
        md, mn = model(lws, tr.Ks[l], int(d.shape[1]), int(d.shape[2]))
        for it in (1, 9):
            def call(l=l, d=d, n=n, md=md, mn=mn, it=it):
                Tl = Tid.clone()
                kernels.icp_track(d, n, md, mn, tr.Ks[l], np.linalg.inv(tr.Ks[l]), Tl, it, max_dist=tr.max_dist[l], min_cos=tr.normal_cos[l],
                                  lm_rel=tr.lm_rel, min_count=tr.min_count, max_rot=tr.max_rot, max_trans=tr.max_trans, scratch=scratch)
            variants["level %d, %d iteration(s)" % (l, it)] = call
    variants["live pyramid (2 halvings, 3 normal maps)"] = lambda: tr.live_pyramid(live)
    variants["track() with cached model maps"] = lambda: tr.track(live, lws, model)
    t = timed(variants, a.reps)
    for name, (m0, m1, mn_) in t.items():
        say("  %-44s %9.1f %9.1f   (min %.1f)" % (name, m0, m1, mn_))
    for l in range(3):
        h, w = int(pyr[l][0].shape[1]), int(pyr[l][0].shape[2])
        per = [(t["level %d, 9 iteration(s)" % l][r] - t["level %d, 1 iteration(s)" % l][r]) / 8.0 for r in (0, 1)]
        floor_us = V * h * w * 32 / (HBM_TBS * 1e12) * 1e6
        say("  level %d (%dx%d): one iteration %.1f / %.1f us; byte floor (32 B per live pixel at %.0f TB/s) %.2f us: %.0f x the floor"
            % (l, w, h, per[0], per[1], HBM_TBS, floor_us, min(per) / floor_us))
    return t


def sibling():
    R = 256
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(512, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=4.0, distributed=False)
    lws = [scene.view_extrinsic(x) for x in (0.0, 40.0, -40.0)]
    ds = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]
    for d, lw in zip(ds, lws):
        sf.integrate(d, lw)
    sf.refresh_samples()
    sv = sf.fs.solver
    Kinv = np.linalg.inv(K)
    start = sv.node_dq.clone()

    def steps(n):
        def call():
            sv.node_dq.copy_(start)
            sv.global_sampled(ds, K, Kinv, lws, scale, center, R / 2, IDENT, 2.0, 0.5, 0.1, n_steps=n, stride=sf.GLOBAL_STRIDE)
        return call
    t = timed({"1 step": steps(1), "9 steps": steps(9)}, a.reps)
    per = [(t["9 steps"][r] - t["1 step"][r]) / 8.0 for r in (0, 1)]
    say("sibling: dfh_gn_global_sampled at config 3 (%d samples, stride %d): 1 step %.1f / %.1f us, 9 steps %.1f / %.1f us: one step %.1f / %.1f us"
        % (int(sv.S), sf.GLOBAL_STRIDE, t["1 step"][0], t["1 step"][1], t["9 steps"][0], t["9 steps"][1], per[0], per[1]))


for cam, angles in CASES:
    track_case(cam, angles)
    torch.cuda.empty_cache()
sibling()
say("not measured: several ranks; the mesh model (render_live); hardware counters")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
