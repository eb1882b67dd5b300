#!/usr/bin/env python3
"""One frame's canonical update, two routes, timed by HIP events (medians, the variants alternating, each timed twice so that
the spread of a variant against itself is on record):
  volume : integrate_depth_views(fresh=...) into the live volume + fuse_volume_dqb in steady state (K1 + K3)
  depth  : integrate_depth_dqb in steady state (K1w: the depth maps through the warp field, no live volume)
at config 3 (256^3, 512 nodes, 3 views of 640x480) and config 5 (512^3, 2 048 nodes, 8 views of 1280x720), float32 volumes;
and what each route does to tracking: the per-frame median of mesh.depth_error(render_live, observed) over ten frames of the
config-5 motion at 128^3 (the sequence of tests/test_gpu_render.py::test_slab_frame_render_live_moving_sequence).
--parent-lib PATH: K1w through this build's library and through the parent commit's (a second CDLL on the same argument structs):
T, Wt and the workspace's index region compared bit for bit over knn 3 / 4 / 8, the three modes (search, search and store, load),
both weight rules, float32 and float64 volumes and maps, a pinhole and a skewed K, on the tests' ragged and main scenes and once at
config 3; then config 3 timed through both, stored indices and search, alternating, two rounds each.
usage: python tools/kbench_integrate_warped.py [--configs 3,5] [--reps 20] [--no-tracking] [--parent-lib build_variants/parent.so] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamicfusion_body_amd import kernels, mesh, scene
from dynamicfusion_body_amd.dq import twist_exp_dq
from dynamicfusion_body_amd.pipeline import SlabFrame

CONFIGS = {3: (256, 512, "C2", (0.0, 40.0, -40.0)), 5: (512, 2048, "C5", tuple(45.0 * v for v in range(8)))}
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-tracking", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def config_scene(cfg):
    """The config's frame: (res, K, Kinv, lws, scale, center, tdist, depths, T0, W0, node tensors P, Q, Wn)."""
    R, N, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(x) for x in angles]
    off = np.array([0.8, -0.5, 0.4]) * 0.5 * scale
    first = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda() for lw in lws]
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda() for lw in lws]
    T0 = torch.empty((R, R, R), dtype=torch.float32, device="cuda")
    W0 = torch.empty_like(T0)
    kernels.integrate_depth_views(T0, W0, first, K, Kinv, lws, scale, center, tdist, fresh=tdist / scale)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    node_dq = twist_exp_dq(np.random.default_rng(0).normal(size=(N, 6)) * np.array([.01, .01, .01, .3, .3, .3]))
    P, Q, Wn = (torch.from_numpy(x).cuda() for x in (node_pos, node_dq, node_w))
    return (R, R, R), K, Kinv, lws, scale, center, tdist, depths, T0, W0, P, Q, Wn


def against_parent(path):
    import parent_lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import warped_np as WN
    plib = parent_lib.open_parent(path, ["dfh_integrate_depth_dqb"])
    say("K1w through this build's library and the parent commit's (%s)" % path)

    def three_modes(lib, shape, knn, N, call):
        """search on a plain workspace, search and store, load: [(T, Wt)] * 3 and the level-1 workspace's bytes."""
        out = []
        with parent_lib.through(lib):
            base = kernels.dqb_workspace(shape)
            ws = kernels.dqb_workspace(shape, knn=knn, n_nodes=N, level=1)
            ws.fill_(-1)
            for w, rebuild in ((base, True), (ws, True), (ws, False)):
                out.append(call(w, rebuild))
        assert ws.numel() > base.numel()
        return out, ws.clone(), base.numel()

    cases = differ = 0
    for name, sc in (("ragged", WN.ragged_scene()), ("main", WN.main_scene())):
        N = len(sc["node_pos"])
        for K, Kinv in ((sc["K"], sc["Kinv"]), WN.skewed(sc["K"])):
            for knn in (3, 4, 8):
                for weight in ("unit", "node_distance"):
                    for vt in (torch.float32, torch.float64):
                        for dt in (torch.float32, torch.float64):
                            depths = [torch.from_numpy(d).to("cuda", dtype=dt) for d in sc["depths"]]

                            def call(ws, rebuild):
                                T0, W0 = WN.start_volumes(sc)
                                T, Wt = torch.from_numpy(T0).to("cuda", dtype=vt), torch.from_numpy(W0).to("cuda", dtype=vt)
                                kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, sc["lws"], sc["scale"], sc["center"], sc["tdist"],
                                                            sc["node_pos"], sc["node_dq"], sc["node_w"], knn, sc["lw_dq"], wmax=7.0,
                                                            weight=weight, tsdf_res=sc["tsdf_res"], workspace=ws, rebuild_candidates=rebuild)
                                return T, Wt
                            (x, wa, nb), (y, wb, _) = three_modes(None, sc["shape"], knn, N, call), three_modes(plib, sc["shape"], knn, N, call)
                            same = all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(x, y)) and torch.equal(wa[nb:], wb[nb:])
                            assert bool((x[0][1] != 0).any())
                            cases += 1
                            if not same:
                                differ += 1
                                say("  DIFFER: %s, %s K, knn %d, %s, volumes %s, maps %s" % (name, "pinhole" if K is sc["K"] else "skewed", knn, weight, vt, dt))
    say("  ragged (13 x 11 x 21) and main (32^3): %d cases x 3 modes, T, Wt and the index region: %s" % (cases, "identical" if not differ else "%d DIFFER" % differ))

    res, K, Kinv, lws, scale, center, tdist, depths, T0, W0, P, Q, Wn = config_scene(3)
    T, Wt = torch.empty_like(T0), torch.empty_like(T0)

    def call3(ws, rebuild):
        T.copy_(T0); Wt.copy_(W0)
        kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, P, Q, Wn, 4, IDENT, weight="node_distance", workspace=ws,
                                    rebuild_candidates=rebuild)
        return T.clone(), Wt.clone()
    (x, wa, nb), (y, wb, _) = three_modes(None, res, 4, P.shape[0], call3), three_modes(plib, res, 4, P.shape[0], call3)
    same = all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(x, y)) and torch.equal(wa[nb:], wb[nb:])
    say("  config 3 (256^3, 512 nodes, 3 views, knn 4, float32, node_distance), 3 modes: %s" % ("identical" if same else "DIFFER"))
    del x, y

    base = kernels.dqb_workspace(res)
    ws = kernels.dqb_workspace(res, knn=4, n_nodes=P.shape[0], level=1)
    call3(base, True); call3(ws, True)
    variants = [(n + who, lib, w) for n, w in (("stored indices", ws), ("search", base)) for who, lib in ((", this build", None), (", parent", plib))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(v[0], rnd): [] for v in variants for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, lib, w in parent_lib.pair_order(variants, rnd):
                T.copy_(T0); Wt.copy_(W0)
                with parent_lib.through(lib):
                    e0.record()
                    kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, P, Q, Wn, 4, IDENT, weight="node_distance",
                                                workspace=w, rebuild_candidates=False)
                    e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    say("  config 3, steady state, medians of %d (us), the variants alternating, each timed in two rounds (a pair swaps places in the second)" % a.reps)
    med = {v[0]: [statistics.median(times[(v[0], rnd)]) for rnd in (0, 1)] for v in variants}
    for n in ("stored indices", "search"):
        parent_lib.verdict(say, "K1w, " + n, med[n + ", this build"], med[n + ", parent"])


def time_config(cfg):
    res, K, Kinv, lws, scale, center, tdist, depths, T0, W0, P, Q, Wn = config_scene(cfg)
    R, N = res[0], P.shape[0]
    H, W = depths[0].shape
    tvox = tdist / scale
    T, Wt, live, live_w = (torch.empty_like(T0) for _ in range(4))
    ws_views = kernels.integrate_workspace(min(len(depths), 16), H, W, res)
    ws_v = kernels.dqb_workspace(res, knn=4, n_nodes=N, level=2)
    ws_d = kernels.dqb_workspace(res, knn=4, n_nodes=N, level=1)

    def volume(rebuild=False):
        kernels.integrate_depth_views(live, live_w, depths, K, Kinv, lws, scale, center, tdist, workspace=ws_views, fresh=tvox)
        kernels.fuse_volume_dqb(T, Wt, live, P, Q, Wn, 4, IDENT, tvox, workspace=ws_v, rebuild_candidates=rebuild)

    def depth(weight, rebuild=False):
        kernels.integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, P, Q, Wn, 4, IDENT, weight=weight,
                                    workspace=ws_d, rebuild_candidates=rebuild)

    variants = [("volume (K1 + K3)", volume), ("depth, node_distance (K1w)", lambda rebuild=False: depth("node_distance", rebuild)),
                ("depth, unit (K1w)", lambda rebuild=False: depth("unit", rebuild))]
    changed = {}
    for name, fn in variants:                       # first calls: search + store; and how many voxels a route updates
        T.copy_(T0); Wt.copy_(W0)
        fn(True)
        changed[name] = int(((T != T0) | (Wt != W0)).sum())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name, _ in variants for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, fn in variants:
                T.copy_(T0); Wt.copy_(W0)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    say("config %d: %d^3, %d nodes, %d views of %dx%d, float32 volumes, steady state, medians of %d (us), each variant timed twice"
        % (cfg, R, N, len(depths), W, H, a.reps))
    for name, _ in variants:
        m0, m1 = statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])
        say("  %-28s %9.1f %9.1f   (min %.1f, voxels changed %d of %d)" % (name, m0, m1, min(times[(name, 0)] + times[(name, 1)]), changed[name], R ** 3))


def tracking():
    R = 128
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    views = [scene.view_extrinsic(0.0), scene.view_extrinsic(120.0)]
    amp = np.array([0.8, -0.5, 0.4])
    say("tracking: config-5 motion at 128^3, 256 nodes, two views, per-frame median |rendered - observed| of the worse view (voxels), frames 1-10")
    for name, kw in (("volume", {}), ("depth, node_distance", dict(update="depth")), ("depth, unit", dict(update="depth", update_weight="unit"))):
        node_pos, node_w = scene.fibonacci_nodes(256, R)
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
        for lw in [scene.view_extrinsic(45.0 * v) for v in range(8)]:
            sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, wall_z=None)).cuda(), lw)
        sf.refresh_samples()
        med, counts = [], []
        for t in range(10):
            off = amp * np.sin(2 * np.pi * (t + 1) / 30.0) * scale
            obs = [scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, wall_z=None, sphere_offset=off) for lw in views]
            counts.append(sf.step([torch.from_numpy(o).cuda() for o in obs], views, gn_iters=10, **kw))
            rendered, _, _ = sf.render_live(views, H, W)
            errs = mesh.depth_error(rendered, torch.from_numpy(np.stack(obs)).cuda(), 0.5 * scale)
            med.append(max(e["median"] for e in errs) / scale)
        say("  %-22s %s   samples %d -> %d" % (name, " ".join("%.3f" % m for m in med), counts[0], counts[-1]))


for c in [int(x) for x in a.configs.split(",") if x]:
    time_config(c)
    torch.cuda.empty_cache()
if not a.no_tracking:
    tracking()
if a.parent_lib:
    against_parent(a.parent_lib)
say("not measured: several ranks (the depth route's saving there is the live sweep's all-gather)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
