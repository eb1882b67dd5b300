#!/usr/bin/env python3
"""K20, the ray cast of a fused volume into the frame's own cameras, timed by HIP events (medians, the variants alternating, each
timed twice so that the spread of a variant against itself is on record):
  (a) plain march                : kernels.raycast without a table
  (b) table build + skipping march: kernels.raycast_table, then kernels.raycast with it (what a caller without a cache pays)
  (c) skipping march, cached table: kernels.raycast with a table built once
  (d) marching cubes + render    : mesh.marching_cubes + mesh.render for the same views (the only route before K20)
  (a') / (c') min_weight 1       : (a) and (c) with the weight volume read too
  (e) no table given             : kernels.raycast as a caller without a table gets it (option raycast_skip unset: by size)
at config 3 (256^3, 3 views of 640x480) and config 5 (512^3, 8 views of 1280x720) on the bench scene, float32 volumes, step 0.5,
refine 1, depth + normals.  With the share of live bricks, the byte floor of one volume read, and -- from the numpy restatement
on every 16th pixel of every 16th row -- the steps a ray has and the samples the plain march evaluates of them.
usage: python tools/kbench_raycast.py [--configs 3,5] [--reps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from dynamicfusion_body_amd import _lib, kernels, mesh, scene

import raycast_np as RN

CONFIGS = {3: (256, "C2", (0.0, 40.0, -40.0)), 5: (512, "C5", tuple(45.0 * v for v in range(8)))}
HBM_TBS = 8.0                                  # nominal peak, for the byte floor only

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def time_config(cfg):
    R, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(x) for x in angles]
    wls = kernels.raycast_inverse_views(lws)
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]
    T = torch.empty((R, R, R), dtype=torch.float32, device="cuda")
    Wt = torch.empty_like(T)
    kernels.integrate_depth_views(T, Wt, depths, K, Kinv, lws, scale, center, tdist, fresh=tdist / scale)
    table = kernels.raycast_table(T)
    live = int(table.sum())
    assert _lib.get_option("raycast_skip") == -1          # unset: a given table is used; without one the wrapper decides by size

    def cast(tab=None, plain=False, **kw):
        if plain:                                         # option 0: never a table (two host calls of a microsecond each)
            _lib.set_option("raycast_skip", 0)
        r = kernels.raycast(T, Wt, K, Kinv, lws, H, W, scale, center, table=tab, wls=wls, **kw)
        if plain:
            _lib.set_option("raycast_skip", None)
        return r

    plain, skip = cast(plain=True), cast(table)
    assert torch.equal(plain.depth, skip.depth) and torch.equal(plain.normals, skip.normals), "the skipping march differs"
    hits = int((plain.depth != 0).sum())
    errs = mesh.depth_error(plain.depth, torch.stack(depths), 1.0 * scale)
    tab2 = torch.empty_like(table)

    def build_and_cast():
        kernels.raycast_table(T, out=tab2)
        cast(tab2)

    def mc_render():
        verts, faces, normals, _ = mesh.marching_cubes(T, 0.0, 1)
        mesh.render(verts, faces, normals, K, lws, H, W, scale=scale, center=center, half=R / 2)

    variants = [("(a) plain march", lambda: cast(plain=True)), ("(b) table + skipping march", build_and_cast),
                ("(c) skipping, cached table", lambda: cast(table)), ("(d) marching cubes + render", mc_render),
                ("(a') plain, min_weight 1", lambda: cast(plain=True, min_weight=1.0)),
                ("(c') skipping, min_weight 1", lambda: cast(table, min_weight=1.0)), ("(e) no table given, option unset", lambda: cast()),
                ("    table build alone", lambda: kernels.raycast_table(T, out=tab2))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name, _ in variants for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, fn in variants:
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    # the walk's statistics: the restatement on every 16th pixel (pixel (x, y) of the small image is pixel (16 x, 16 y))
    sub = 16
    Ks = Kinv @ np.diag([float(sub), float(sub), 1.0])
    Tn, Wn = T.cpu().numpy(), Wt.cpu().numpy()
    st = RN.raycast(Tn, Wn, Ks, wls, (H + sub - 1) // sub, (W + sub - 1) // sub, scale, center)
    floor_us = R ** 3 * 4 / (HBM_TBS * 1e12) * 1e6
    say("config %d: %d^3 float32, %d views of %dx%d, step 0.5, refine 1, depth + normals, medians of %d (us), each variant timed twice"
        % (cfg, R, len(lws), W, H, a.reps))
    say("  rays %d, hits %d (%.1f %%); live bricks %d of %d (%.1f %%); median |cast - input depth| %s voxels"
        % (len(lws) * H * W, hits, 100.0 * hits / (len(lws) * H * W), live, table.numel(), 100.0 * live / table.numel(),
           ", ".join("%.3f" % (e["median"] / scale) for e in errs)))
    say("  per ray (restatement, every %dth pixel): steps %.1f, samples evaluated by the plain march %.1f"
        % (sub, float(st["steps"].mean()), float(st["samples"].mean())))
    say("  byte floor of one volume read at %.0f TB/s: %.1f us" % (HBM_TBS, floor_us))
    med = {}
    for name, _ in variants:
        m0, m1 = statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])
        med[name] = (m0, m1)
        say("  %-30s %10.1f %10.1f   (min %.1f; %.1f x the byte floor)" % (name, m0, m1, min(times[(name, 0)] + times[(name, 1)]),
                                                                          min(m0, m1) / floor_us))
    pa, pb = med["(a) plain march"], med["(b) table + skipping march"]
    spread = max(abs(pa[0] - pa[1]), abs(pb[0] - pb[1]))
    gain = min(pa) - max(pb)
    say("  (b) against (a): %.1f us %s, spread between a variant's two timings %.1f us: %s"
        % (abs(gain), "faster" if gain > 0 else "slower", spread, "skipping wins" if gain > spread else "no win: plain march"))


for c in [int(x) for x in a.configs.split(",") if x]:
    time_config(c)
    torch.cuda.empty_cache()
say("not measured: several ranks; float64 volumes; hardware counters; the samples the skipping march evaluates per ray (the kernel "
    "keeps no counters: the share of live bricks stands in for it)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
