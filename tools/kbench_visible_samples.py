#!/usr/bin/env python3
"""The solve's two sample sources side by side, timed by HIP events (medians, the variants alternating, each timed twice so that
the spread of a variant against itself is on record):
  band        : every band voxel of the canonical volume (extract_surface_samples), today's default
  visible /s  : the rendered model (SlabFrame.visible_samples, mesh.render_samples) at pixel stride s = 1, 2
at config 3 (256^3, 512 nodes, 3 views of 640x480) and config 5 (512^3, 2 048 nodes, 8 views of 1280x720), float32 volumes:
the sample count, the refresh stage by stage, one frame's solve (two rigid-mode steps + ten GN iterations, step()'s defaults)
from the same warp field, and the whole step(); then what each source does to tracking: the per-frame median of
mesh.depth_error(render_live, observed) over ten frames of the config-5 motion at 128^3 (the sequence of
tests/test_gpu_render_samples.py::test_slab_frame_moving_sequence_band_and_visible).
--band: the band source's |T| bound in voxels at the two configs (default 4, SlabFrame's and the bench frame's; the tracking
sequence keeps the frame tests' band of 2).
--parent-lib PATH: per config, mesh.render_samples at both strides with the count (its scan) and the emit pass through this
build's library and through the parent commit's (tools/parent_lib.py): positions, normals and pixels compared bit for bit, then
both timed, alternating, two rounds each.
usage: python tools/kbench_visible_samples.py [--configs 3,5] [--band 4] [--reps 20] [--no-tracking] [--parent-lib PATH] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamicfusion_body_amd import _lib, mesh, scene
from dynamicfusion_body_amd.device import HostScalar, current_stream_ptr
from dynamicfusion_body_amd.pipeline import SlabFrame, extract_surface_samples
from dynamicfusion_body_amd.solve import sample_knn, warp_points

CONFIGS = {3: (256, 512, "C2", (0.0, 40.0, -40.0)), 5: (512, 2048, "C5", tuple(45.0 * v for v in range(8)))}
VARIANTS = (("band", None), ("visible /1", 1), ("visible /2", 2))

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="3,5")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--band", type=float, default=4.0)
ap.add_argument("--no-tracking", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Stages:
    """Events between the stages of one refresh; us per stage once the device has drained."""

    def __init__(self):
        self.names, self.ev = [], [torch.cuda.Event(enable_timing=True)]
        self.ev[0].record()

    def __call__(self, name):
        self.names.append(name)
        self.ev.append(torch.cuda.Event(enable_timing=True))
        self.ev[-1].record()

    def us(self):
        torch.cuda.synchronize()
        return {n: self.ev[i].elapsed_time(self.ev[i + 1]) * 1e3 for i, n in enumerate(self.names)}


def solver_stages(sf, pos, nrm, st):
    sv = sf.fs.solver
    nbr, wts = sample_knn(pos, sv.node_pos, sv.node_w, sf.knn, bricks=sf.knn_bricks)
    st("sample knn")
    sv.set_samples(pos, nrm, nbr=nbr, weights=wts)
    st("sort")
    sv.prepare()
    st("plan")


def refresh_band(sf):
    st = Stages()
    pos, nrm = extract_surface_samples(sf.T, sf.Wt, sf.band, x0=sf.a)
    st("extract (count, scan, emit)")
    solver_stages(sf, pos, nrm, st)
    return st.us()


def refresh_visible(sf, lws, H, W, stride):
    """SlabFrame.visible_samples + refresh_samples, with an event after every stage (the library calls of mesh.render_samples
    one by one)."""
    lib = _lib.load()
    sv = sf.fs.solver
    st = Stages()
    verts, faces, normals, _ = mesh.marching_cubes(sf.T, 0.0, 1)
    st("marching cubes")
    nbr, _ = sample_knn(verts, sv.node_pos, sv.node_w, sf.knn)
    st("vertex knn")
    warped, _ = warp_points(verts, normals, sf.ident_lw, nbr=nbr, node_dq=sv.node_dq, node_pos=sv.node_pos, node_w=sv.node_w)
    st("warp")
    Kf, lwf, nv = mesh._view_table(sf.K, lws)
    V, P, N = warped.contiguous(), verts.to(torch.float64).contiguous(), normals.to(torch.float64).contiguous()
    F = faces.to(torch.int32).contiguous()
    wsp = mesh.render_workspace(nv, H, W, F.shape[0])
    Ka, La, Ca = _lib.darr(Kf, 9 * nv), _lib.darr(lwf, 12 * nv), _lib.darr(np.broadcast_to(sf.center, (3,)), 3)
    ws, nbytes = wsp.buf.data_ptr(), wsp.buf.numel() * 8
    geom = (float(sf.scale), Ca, float(sf.R / 2), 1e-3)
    st("convert, allocate")
    _lib.check(lib.dfh_render_raster(V.data_ptr(), V.shape[0], F.data_ptr(), F.shape[0], nv, Ka, La, H, W, *geom, ws, nbytes,
                                     current_stream_ptr()), "dfh_render_raster")
    st("raster")
    sbytes = lib.dfh_render_samples_workspace_bytes(nv, H, W, stride)
    scan = torch.empty((sbytes + 7) // 8, dtype=torch.int64, device="cuda")
    total = HostScalar(torch.int64)
    _lib.check(lib.dfh_render_samples_count(nv, H, W, F.shape[0], stride, ws, nbytes, scan.data_ptr(), scan.numel() * 8, total.ptr(),
                                            current_stream_ptr()), "dfh_render_samples_count")
    n = total.get()
    st("count (+ read-back)")
    pos = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    pix = torch.empty((n,), dtype=torch.int64, device="cuda")
    _lib.check(lib.dfh_render_samples_emit(V.data_ptr(), P.data_ptr(), N.data_ptr(), V.shape[0], F.data_ptr(), F.shape[0], nv, Ka, La, H, W,
                                           *geom, stride, ws, nbytes, scan.data_ptr(), scan.numel() * 8, pos.data_ptr(), nrm.data_ptr(),
                                           pix.data_ptr(), n, current_stream_ptr()), "dfh_render_samples_emit")
    st("emit (compact + rows)")
    solver_stages(sf, pos, nrm, st)
    return st.us()


def fuse_views(K, H, W):
    """The eight views every frame of this tool fuses its canonical volume from: [(depth map, lw)], rendered once."""
    lws = [scene.view_extrinsic(45.0 * v) for v in range(8)]
    return [(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, wall_z=None)).cuda(), lw) for lw in lws]


def make_frame(R, N, K, fuse, band=2.0):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=band, distributed=False)
    for depth, lw in fuse:
        sf.integrate(depth, lw)
    sf.refresh_samples()
    return sf, scale


def medians(times, name):
    return statistics.median(times[(name, 0)]), statistics.median(times[(name, 1)])


def time_config(cfg):
    R, N, cam, angles = CONFIGS[cfg]
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    lws = [scene.view_extrinsic(x) for x in angles]
    fuse = fuse_views(K, H, W)
    frames = {}
    for name, stride in VARIANTS:
        frames[name], scale = make_frame(R, N, K, fuse, a.band)
        if stride is not None:
            frames[name].set_sample_source("visible", lws, (H, W), stride=stride)
    off = np.array([0.8, -0.5, 0.4]) * 0.5 * scale
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, wall_z=None, sphere_offset=off)).cuda()
              for lw in lws]
    say("config %d: %d^3, %d nodes, %d views of %dx%d, float32 volumes, band %g, medians of %d (us), each variant timed twice"
        % (cfg, R, N, len(lws), W, H, a.band, a.reps))
    # -- the refresh, stage by stage, from the static state
    stage_t = {(name, rnd): [] for name, _ in VARIANTS for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, stride in VARIANTS:
                us = refresh_band(frames[name]) if stride is None else refresh_visible(frames[name], lws, H, W, stride)
                if rep >= 2:
                    stage_t[(name, rnd)].append(us)
    for name, _ in VARIANTS:
        say("  refresh, %s: S = %d" % (name, frames[name].fs.solver.S))
        tot = [0.0, 0.0]
        for stage in stage_t[(name, 0)][0]:
            m = [statistics.median(u[stage] for u in stage_t[(name, rnd)]) for rnd in (0, 1)]
            tot = [tot[0] + m[0], tot[1] + m[1]]
            say("    %-30s %9.1f %9.1f" % (stage, m[0], m[1]))
        say("    %-30s %9.1f %9.1f" % ("sum", tot[0], tot[1]))
    # -- one frame's solve from the same (identity) field: step()'s defaults
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {(name, rnd): [] for name, _ in VARIANTS for rnd in (0, 1)}
    for rep in range(a.reps + 2):
        for rnd in (0, 1):
            for name, _ in VARIANTS:
                sf = frames[name]
                dq0 = sf.fs.solver.node_dq.clone()
                sf.fs.solver.prepare()
                torch.cuda.synchronize()
                e0.record()
                sf.fs.global_iteration(depths, lws, max_dist=2.0, huber=0.5, lm_rel=0.1, n_iters=sf.GLOBAL_ITERS, stride=sf.GLOBAL_STRIDE)
                sf.fs.gn_iteration(depths, lws, rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.5, n_iters=10)
                e1.record()
                torch.cuda.synchronize()
                sf.fs.solver.node_dq.copy_(dq0)
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    for name, _ in VARIANTS:
        say("  solve (2 rigid + 10 GN), %-12s %9.1f %9.1f" % ((name,) + medians(times, name)))
    # -- the whole step(), steady state on the moved scene
    times = {(name, rnd): [] for name, _ in VARIANTS for rnd in (0, 1)}
    counts = {}
    for rep in range(a.reps + 3):
        for rnd in (0, 1):
            for name, _ in VARIANTS:
                torch.cuda.synchronize()
                e0.record()
                counts[name] = frames[name].step(depths, lws, gn_iters=10)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    for name, _ in VARIANTS:
        say("  step(), %-28s %9.1f %9.1f   (S = %d at the end)" % ((name,) + medians(times, name) + (counts[name],)))
    if a.parent_lib:
        import parent_lib
        sf = frames["band"]
        verts, faces, normals, _ = mesh.marching_cubes(sf.T, 0.0, 1)
        wsp = mesh.render_workspace(len(lws), H, W, faces.shape[0])
        for stride in (1, 2):
            parent_lib.against_parent(say, "  render_samples /%d" % stride,
                                      lambda lib: mesh.render_samples(verts, faces, verts, normals, sf.K, lws, H, W, sf.scale, sf.center, sf.R / 2,
                                                                      stride=stride, workspace=wsp),
                                      ["dfh_render_samples_count", "dfh_render_samples_emit"], a.parent_lib, a.reps)


def tracking():
    R = 128
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    views = [scene.view_extrinsic(0.0), scene.view_extrinsic(120.0)]
    amp = np.array([0.8, -0.5, 0.4])
    say("tracking: config-5 motion at 128^3, 256 nodes, two views, per-frame median |rendered - observed| of the worse view (voxels), frames 1-10")
    fuse = fuse_views(K, H, W)
    for name, stride in VARIANTS:
        sf, scale = make_frame(R, 256, K, fuse)
        if stride is not None:
            sf.set_sample_source("visible", views, (H, W), stride=stride)
        med, counts = [], []
        for t in range(10):
            off = amp * np.sin(2 * np.pi * (t + 1) / 30.0) * scale
            obs = [scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, wall_z=None, sphere_offset=off) for lw in views]
            counts.append(sf.step([torch.from_numpy(o).cuda() for o in obs], views, gn_iters=10))
            rendered, _, _ = sf.render_live(views, H, W)
            errs = mesh.depth_error(rendered, torch.from_numpy(np.stack(obs)).cuda(), 0.5 * scale)
            med.append(max(e["median"] for e in errs) / scale)
        say("  %-12s %s   worst %.3f   samples %d -> %d" % (name, " ".join("%.3f" % m for m in med), max(med), counts[0], counts[-1]))


for c in [int(x) for x in a.configs.split(",") if x]:
    time_config(c)
    torch.cuda.empty_cache()
if not a.no_tracking:
    tracking()
say("not measured: several ranks (the visible source is single rank)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
