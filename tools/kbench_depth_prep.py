#!/usr/bin/env python3
"""The depth preprocessing kernel (kernels.depth_prep: bilateral filter + normal map + mask, one launch for all views of a frame),
timed by HIP events round the call (medians, the variants alternating, each timed twice so that the spread of a variant against
itself is on record) on config 3's maps (3 x 480 x 640) and config 5's (8 x 720 x 1280): radii 1, 3 and 6, float32 and float64
inputs, and the two layouts of the normals' stores (option k12_store: 0 = three strided dword stores per lane, 1 = re-laid
through LDS into runs of consecutive dwords).  Every time stands beside the byte floor of 20 B per pixel (4 B read, 16 B
written) and the rate that floor would need, as a fraction of the copy ceiling bench.py measures (tools/ubench/rmw_stream, run
here as a child process in the same session) and of the 8 TB/s of the data sheet.
Then SlabFrame.step() with and without the stage at both configs, alternating.
usage: python tools/kbench_depth_prep.py [--configs 3,5] [--reps 20] [--no-step] [--no-ceiling] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {3: (256, 512, "C2", (0.0, 40.0, -40.0)), 5: (512, 2048, "C5", tuple(45.0 * v for v in range(8)))}
RADII = (1, 3, 6)
HBM_PEAK_GBS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--no-ceiling", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def copy_ceiling():
    """bench.py's copy ceiling (GB/s): the best in-place read-modify-write rate of tools/ubench/rmw_stream at 512^3."""
    ub = os.path.join(ROOT, "tools", "ubench", "rmw_stream")
    r = subprocess.run([ub, "512", "ceiling"], capture_output=True, text=True, timeout=120)
    c = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return max(c["rmw_rows_GBps"], c["rmw_rows_nt_GBps"], c["rmw_bricks_4x2x32_GBps"], c["rmw_bricks_4x2x32_nt_GBps"])


ceiling = None
if not a.no_ceiling:                                   # (before this process opens the device)
    try:
        ceiling = copy_ceiling()
    except Exception as e:
        say("copy ceiling not measured: %s: %s" % (type(e).__name__, str(e)[:160]))

import torch  # noqa: E402
from dynamicfusion_body_amd import _lib, kernels, scene  # noqa: E402
from dynamicfusion_body_amd.depth_prep import DepthPrep  # noqa: E402
from dynamicfusion_body_amd.pipeline import SlabFrame  # noqa: E402


def noisy_maps(K, lws, H, W, dtype, offset=None):
    rng = np.random.default_rng(7)
    out = []
    for lw in lws:
        d = scene.render_depth(K, lw, H, W, dtype=np.float64, invalid_frac=0.02, sphere_offset=offset)
        d = np.where(d < 0, d + rng.normal(0.0, 0.003, size=d.shape), 0.0)
        out.append(torch.from_numpy(d.astype(dtype)).cuda())
    return out


def time_kernel(cfg):
    R, N, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    lws = [scene.view_extrinsic(x) for x in angles]
    V = len(lws)
    maps = {dt: noisy_maps(K, lws, H, W, dt) for dt in (np.float32, np.float64)}
    out = (torch.empty((V, H, W), dtype=torch.float32, device="cuda"), torch.empty((V, H, W, 3), dtype=torch.float32, device="cuda"))
    floor = 20.0 * V * H * W
    variants = [(r, dt, st) for r in RADII for dt in (np.float32, np.float64) for st in (0, 1)]
    preps = {r: DepthPrep(radius=r, sigma_s=max(1.0, r / 2.0)) for r in RADII}
    tabs = {r: preps[r].tables("cuda") for r in RADII}

    def call(r, dt, st):
        _lib.set_option("k12_store", st)
        kernels.depth_prep(maps[dt], Kinv, tabs[r], preps[r].max_jump, preps[r].min_cos, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(v, rnd): [] for v in variants for rnd in (0, 1)}
    kept = {}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for v in variants:
                e0.record()
                call(*v)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(v, rnd)].append(e0.elapsed_time(e1) * 1e3)
                elif rep == 0 and rnd == 0:
                    kept[v] = (int((out[0] != 0).sum()), out[0].clone(), out[1].clone())
    _lib.set_option("k12_store", None)
    say("config %d maps: %d views of %dx%d, 3 mm noise; byte floor %.1f MB (20 B per pixel); medians of %d (us), each variant timed twice"
        % (cfg, V, W, H, floor / 1e6, a.reps))
    say("  %-34s %9s %9s %9s  %s" % ("radius, input, normal stores", "us", "us", "min", "floor rate GB/s (of copy ceiling%s, of 8 TB/s)"
                                     % ("" if ceiling is None else " %.0f GB/s" % ceiling)))
    for v in variants:
        r, dt, st = v
        m0, m1 = statistics.median(times[(v, 0)]), statistics.median(times[(v, 1)])
        rate = floor / (min(m0, m1) * 1e-6) / 1e9
        same = torch.equal(kept[v][1], kept[(r, dt, 0)][1]) and torch.equal(kept[v][2], kept[(r, dt, 0)][2])
        say("  r=%d %-8s %-20s %9.1f %9.1f %9.1f  %7.0f (%s, %.2f)  kept %d px%s"
            % (r, np.dtype(dt).name, "strided dwords" if st == 0 else "re-laid through LDS", m0, m1, min(times[(v, 0)] + times[(v, 1)]), rate,
               "n/a" if ceiling is None else "%.2f" % (rate / ceiling), rate / HBM_PEAK_GBS, kept[v][0], "" if same else "  LAYOUTS DIFFER"))


def time_step(cfg):
    R, N, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    lws = [scene.view_extrinsic(x) for x in angles]
    scale, center, tdist = scene.grid_params(R)
    first = noisy_maps(K, lws, H, W, np.float32)
    off = np.array([0.8, -0.5, 0.4]) * 0.5 * scale
    depths = noisy_maps(K, lws, H, W, np.float32, offset=off)
    frames = {}
    for name, p in (("raw maps", None), ("depth_prep (defaults)", DepthPrep())):
        node_pos, node_w = scene.fibonacci_nodes(N, R)
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False, depth_prep=p)
        for d, lw in zip(first if p is None else p(first, sf.Kinv)[0], lws):
            sf.integrate(d, lw)
        sf.refresh_samples()
        frames[name] = sf
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name in frames for rnd in (0, 1)}
    counts = {}
    for rep in range(a.reps + 3):
        for rnd in (0, 1):
            for name, sf in frames.items():
                torch.cuda.synchronize()
                e0.record()
                counts[name] = sf.step(depths, lws, gn_iters=10)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    ms = {}
    frames["depth_prep (defaults)"].step(depths, lws, gn_iters=10, stage_ms=ms)
    say("config %d: SlabFrame.step(), %d^3, %d nodes, %d views of %dx%d, steady state, medians of %d (us), each variant timed twice"
        % (cfg, R, N, len(lws), W, H, a.reps))
    for name in frames:
        say("  step(), %-24s %9.1f %9.1f   (S = %d at the end)" % (name, statistics.median(times[(name, 0)]),
                                                                  statistics.median(times[(name, 1)]), counts[name]))
    say("  one synchronised step with depth_prep, stage by stage (ms): " + ", ".join("%s %.2f" % kv for kv in ms.items()))


cfgs = [int(x) for x in a.configs.split(",") if x]
for c in cfgs:
    time_kernel(c)
if not a.no_step:
    for c in cfgs:
        time_step(c)
        torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
