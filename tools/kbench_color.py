#!/usr/bin/env python3
"""K17, the colour call of one frame beside the frame's depth-driven canonical update, timed by HIP events (medians, the variants
alternating, each timed twice so that the spread of a variant against itself is on record):
  K1w            : integrate_depth_dqb in steady state (stored indices): the chain on EVERY voxel
  colour, stored : integrate_color with the stored indices: the same chain behind the canonical gate
  colour, search : integrate_color searching the bricks' candidate lists (a plain workspace)
  colour, none   : integrate_color without nodes
  sample_colors  : the colour volume sampled at the vertices of the canonical mesh
at config 3 (256^3, 512 nodes, 3 views of 640x480) and config 5 (512^3, 2 048 nodes, 8 views of 1280x720), float32 volumes, a
band of 1.5 voxels; with the live-voxel share (the voxels that pass the canonical gate) and the coloured share.  And
SlabFrame.step(update="depth") with and without colours at config 3 (host clock around a synchronised step).
--parent-lib PATH: integrate_color through this build's library and through the parent commit's (a second CDLL on the same argument
structs): C compared bit for bit over knn 3 / 4 / 8, the three modes (none, search, stored) and a pinhole and a skewed K on the
tests' ragged and main scenes and once at config 3; then config 3 timed through both, alternating, two rounds each.
usage: python tools/kbench_color.py [--configs 3,5] [--reps 20] [--no-step] [--parent-lib build_variants/parent.so] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamicfusion_body_amd import kernels, mesh, scene
from dynamicfusion_body_amd.dq import twist_exp_dq
from dynamicfusion_body_amd.pipeline import SlabFrame

CONFIGS = {3: (256, 512, "C2", (0.0, 40.0, -40.0)), 5: (512, 2048, "C5", tuple(45.0 * v for v in range(8)))}
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
BAND = 1.5

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def scene_of(cfg):
    R, N, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(x) for x in angles]
    off = np.array([0.8, -0.5, 0.4]) * 0.5 * scale
    first = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda() for lw in lws]
    g = torch.Generator().manual_seed(cfg)
    colors = [torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=g).cuda() for _ in lws]
    return R, N, H, W, K, scale, center, tdist, lws, first, depths, colors


def time_config(cfg):
    R, N, H, W, K, scale, center, tdist, lws, first, depths, colors = scene_of(cfg)
    Kinv = np.linalg.inv(K)
    tvox = tdist / scale
    res = (R, R, R)
    T0 = torch.empty(res, dtype=torch.float32, device="cuda")
    W0 = torch.empty_like(T0)
    kernels.integrate_depth_views(T0, W0, first, K, Kinv, lws, scale, center, tdist, fresh=tvox)
    T, Wt = torch.empty_like(T0), torch.empty_like(T0)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    rng = np.random.default_rng(0)
    node_dq = twist_exp_dq(rng.normal(size=(N, 6)) * np.array([.01, .01, .01, .3, .3, .3]))
    P, Q, Wn = (torch.from_numpy(x).cuda() for x in (node_pos, node_dq, node_w))
    ws = kernels.dqb_workspace(res, knn=4, n_nodes=N, level=1)
    ws_plain = kernels.dqb_workspace(res)
    kernels.dqb_build_candidates(ws_plain, res, P, 4)
    C = kernels.color_volume(res)

    def k1w(rebuild=False):
        kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, P, Q, Wn, 4, IDENT, weight="node_distance",
                                    workspace=ws, rebuild_candidates=rebuild)

    def color(mode):
        kw = {} if mode == "none" else dict(node_pos=P, node_dq=Q, node_w=Wn, knn=4, lw_dq=IDENT)
        if mode == "stored":
            kw.update(workspace=ws, stored_indices=True)
        elif mode == "search":
            kw.update(workspace=ws_plain)
        kernels.integrate_color(C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, BAND, **kw)

    # the frame's state: the canonical volume after this frame's update (first call: search + store)
    T.copy_(T0); Wt.copy_(W0)
    k1w(True)
    Tf, Wf = T.clone(), Wt.clone()
    live = int(((Wf > 0) & (Tf.abs() <= BAND)).sum())
    C.zero_()
    color("stored")
    coloured = int((C[..., 3] > 0).sum())
    Cs = C.clone()
    for mode in ("search", "none"):                 # (the searching mode gives the stored mode's bits)
        C.zero_()
        color(mode)
        if mode == "search":
            assert torch.equal(C, Cs), "search and stored modes differ"
    verts, faces, _, _ = mesh.marching_cubes(Tf, 0.0, 1)
    pts = verts.double().contiguous()
    C.copy_(Cs)
    rgb, valid = kernels.sample_colors(C, pts)
    n_valid = int(valid.sum())

    def sample():
        kernels.sample_colors(C, pts)

    variants = [("K1w, stored indices", lambda: k1w(), True), ("colour, stored indices", lambda: color("stored"), False),
                ("colour, search", lambda: color("search"), False), ("colour, no nodes", lambda: color("none"), False),
                ("sample_colors", sample, False)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name, _, _ in variants for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, fn, writes_volume in variants:
                if writes_volume:
                    T.copy_(T0); Wt.copy_(W0)
                else:
                    T.copy_(Tf); Wt.copy_(Wf)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    say("config %d: %d^3, %d nodes, %d views of %dx%d, float32 volumes, band %.1f voxels, steady state, medians of %d (us), each "
        "variant timed twice" % (cfg, R, N, len(depths), W, H, BAND, a.reps))
    say("  live voxels (w > 0, |T| <= band) %d of %d = %.2f %%; coloured %d; mesh %d vertices, %d coloured"
        % (live, R ** 3, 100.0 * live / R ** 3, coloured, pts.shape[0], n_valid))
    for name, _, _ in variants:
        m0, m1 = statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])
        say("  %-24s %9.1f %9.1f   (min %.1f)" % (name, m0, m1, min(times[(name, 0)] + times[(name, 1)])))


def against_parent(path):
    import parent_lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import color_np as CN
    import warped_np as WN
    plib = parent_lib.open_parent(path, ["dfh_integrate_color"])
    say("integrate_color through this build's library and the parent commit's (%s)" % path)

    def color(lib, C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, mode, nodes, ws, ws_plain, **kw):
        if mode == "stored":
            kw.update(nodes, workspace=ws, stored_indices=True)
        elif mode == "search":
            kw.update(nodes, workspace=ws_plain)
        with parent_lib.through(lib):
            kernels.integrate_color(C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, BAND, **kw)

    cases = differ = 0
    for name, sc in (("ragged", WN.ragged_scene()), ("main", WN.main_scene())):
        N = len(sc["node_pos"])
        colors = kernels.color_images(CN.color_images(sc))
        depths = [torch.from_numpy(d).cuda() for d in sc["depths"]]
        start = torch.from_numpy(CN.pattern(sc["shape"])).cuda()
        for K, Kinv in ((sc["K"], sc["Kinv"]), WN.skewed(sc["K"])):
            for knn in (3, 4, 8):
                nodes = dict(node_pos=sc["node_pos"], node_dq=sc["node_dq"], node_w=sc["node_w"], knn=knn, lw_dq=sc["lw_dq"])
                ws = kernels.dqb_workspace(sc["shape"], knn=knn, n_nodes=N, level=1)
                T0, W0 = WN.start_volumes(sc, np.float32)
                T, Wt = torch.from_numpy(T0).cuda(), torch.from_numpy(W0).cuda()            # the frame's canonical volume and its indices
                kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, sc["lws"], sc["scale"], sc["center"], sc["tdist"], sc["node_pos"],
                                            sc["node_dq"], sc["node_w"], knn, sc["lw_dq"], tsdf_res=sc["tsdf_res"], workspace=ws)
                ws_plain = ws[:kernels.dqb_workspace(sc["shape"]).numel()].clone()
                for mode in ("none", "search", "stored"):
                    got = []
                    for lib in (None, plib):
                        C = start.clone()
                        color(lib, C, T, Wt, depths, colors, K, Kinv, sc["lws"], sc["scale"], sc["center"], sc["tdist"], mode, nodes, ws, ws_plain,
                              tsdf_res=sc["tsdf_res"])
                        got.append(C)
                    assert not torch.equal(got[0], start)
                    cases += 1
                    if not torch.equal(got[0], got[1]):
                        differ += 1
                        say("  DIFFER: %s, %s K, knn %d, %s" % (name, "pinhole" if K is sc["K"] else "skewed", knn, mode))
    say("  ragged (13 x 11 x 21) and main (32^3): %d cases, C: %s" % (cases, "identical" if not differ else "%d DIFFER" % differ))

    R, N, H, W, K, scale, center, tdist, lws, first, depths, colors = scene_of(3)
    Kinv = np.linalg.inv(K)
    T = torch.empty((R, R, R), dtype=torch.float32, device="cuda")
    Wt = torch.empty_like(T)
    kernels.integrate_depth_views(T, Wt, first, K, Kinv, lws, scale, center, tdist, fresh=tdist / scale)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    node_dq = twist_exp_dq(np.random.default_rng(0).normal(size=(N, 6)) * np.array([.01, .01, .01, .3, .3, .3]))
    P, Q, Wn = (torch.from_numpy(x).cuda() for x in (node_pos, node_dq, node_w))
    nodes = dict(node_pos=P, node_dq=Q, node_w=Wn, knn=4, lw_dq=IDENT)
    ws = kernels.dqb_workspace((R, R, R), knn=4, n_nodes=N, level=1)
    kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, P, Q, Wn, 4, IDENT, weight="node_distance", workspace=ws)
    ws_plain = ws[:kernels.dqb_workspace((R, R, R)).numel()].clone()
    C = kernels.color_volume((R, R, R))
    same = []
    for mode in ("none", "search", "stored"):
        got = []
        for lib in (None, plib):
            C.zero_()
            color(lib, C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, mode, nodes, ws, ws_plain)
            got.append(C.clone())
        assert bool((got[0][..., 3] > 0).any())
        same.append(torch.equal(got[0], got[1]))
    say("  config 3 (256^3, 512 nodes, 3 views, knn 4), none / search / stored, C: %s" % ("identical" if all(same) else "DIFFER %s" % same))
    del got

    variants = [(m + who, lib, m) for m in ("none", "search", "stored") for who, lib in ((", this build", None), (", parent", plib))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(v[0], rnd): [] for v in variants for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, lib, mode in parent_lib.pair_order(variants, rnd):
                e0.record()
                color(lib, C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, mode, nodes, ws, ws_plain)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    say("  config 3, steady state, medians of %d (us), the variants alternating, each timed in two rounds (a pair swaps places in the second)" % a.reps)
    med = {v[0]: [statistics.median(times[(v[0], rnd)]) for rnd in (0, 1)] for v in variants}
    for m in ("none", "search", "stored"):
        parent_lib.verdict(say, "colour, " + m, med[m + ", this build"], med[m + ", parent"])


def time_step(cfg=3, frames=12):
    R, N, H, W, K, scale, center, tdist, lws, first, depths, colors = scene_of(cfg)
    say("SlabFrame.step(update='depth', gn_iters=10) at config %d, host clock around a synchronised step, medians of %d frames (ms), "
        "each variant timed twice, alternating" % (cfg, frames - 2))
    loops = {}
    for name in ("without colours", "with colours"):
        node_pos, node_w = scene.fibonacci_nodes(N, R)
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False,
                       color_band=BAND if name == "with colours" else None)
        for d, lw in zip(first, lws):
            sf.integrate(d, lw)
        sf.refresh_samples()
        loops[name] = sf
    times = {(name, rnd): [] for name in loops for rnd in (0, 1)}
    for f in range(frames):
        for rnd in (0, 1):
            for name, sf in loops.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sf.step(depths, lws, gn_iters=10, update="depth", colors=colors if name == "with colours" else None)
                torch.cuda.synchronize()
                if f >= 2:
                    times[(name, rnd)].append((time.perf_counter() - t0) * 1e3)
    for name in loops:
        say("  %-24s %9.3f %9.3f" % (name, statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])))


for c in [int(x) for x in a.configs.split(",") if x]:
    time_config(c)
    torch.cuda.empty_cache()
if not a.no_step:
    time_step()
if a.parent_lib:
    against_parent(a.parent_lib)
say("not measured: several ranks; hardware counters (the split of the colour call between the gate's two loads and the live lanes' chain)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
