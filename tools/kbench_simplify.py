#!/usr/bin/env python3
"""K24, mesh simplification by vertex clustering with quadrics, timed by HIP events (medians of --reps runs after a warm-up run;
each line's spread against itself is printed as min .. max) on
  config 3 : the marching-cubes mesh of the config-3 scene (256^3, 3 views of camera C2)
  config 5 : the marching-cubes mesh of the config-5 scene (512^3, the 8-view orbit of camera C5)
per mesh and cell (2 and 4 voxels): the stages of one mesh.simplify call with the normals as an attribute -- keys (it
synchronises, so the events bracket a host wait too), the two stable torch.sorts, grouping, vertex quadrics + clusters, the
attribute, faces + compaction -- the whole call in both modes, the share of the sorts, face counts before and after, the
fall-back count, mesh.compare_meshes of the simplified against the original in both modes, and beside them marching_cubes on
the same volume and mesh.filter_components on the same mesh in the same run.
usage: python tools/kbench_simplify.py [--reps 30] [--no-512] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamicfusion_body_amd import FusionDM, _lib, mesh, scene
from dynamicfusion_body_amd.device import current_stream_ptr, dtype_code
from dynamicfusion_body_amd.pipeline import SlabFrame

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--no-512", action="store_true")
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


def config3_volume(R=256):                                  # (the two scene volumes of kbench_components.py)
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


def stages(v, f, nrm, cell, mode):
    """One simplify call, stage by stage, through the library's entry points as mesh.simplify issues them."""
    lib = _lib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    org = (ctypes.c_double * 3)(*[float(x) for x in v.double().amin(dim=0).cpu().numpy()])
    ws = torch.empty((lib.dfh_mesh_simplify_workspace_bytes(V, F) + 7) // 8, dtype=torch.int64, device=dev)
    wsb, S = ws.numel() * 8, current_stream_ptr()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    st = {}

    def do_keys():
        _lib.check(lib.dfh_mesh_simplify_keys(v.data_ptr(), dtype_code(v), V, f.data_ptr(), F, cell, org, keys.data_ptr(), ws.data_ptr(), wsb, S), "keys")

    def do_sorts():
        st["skeys"], st["order"] = torch.sort(keys, stable=True)
        st["scv"], st["corder"] = torch.sort(f.reshape(-1), stable=True)

    vclus, cstart, ccount, cbeg, cend = i32(V), i32(V), i32(V), i32(V), i32(V)
    n = ctypes.c_long(0)

    def do_group():
        _lib.check(lib.dfh_mesh_simplify_group(st["skeys"].data_ptr(), st["order"].data_ptr(), V, st["scv"].data_ptr(), F, vclus.data_ptr(), cstart.data_ptr(),
                                               ccount.data_ptr(), cbeg.data_ptr(), cend.data_ptr(), ctypes.byref(n), ws.data_ptr(), wsb, S), "group")

    out = {}
    out["keys"] = timed(do_keys)
    out["sorts"] = timed(do_sorts)
    out["group"] = timed(do_group)
    C = int(n.value)
    cverts = torch.empty((C, 3), dtype=v.dtype, device=dev)
    cn = torch.empty((C, 3), dtype=nrm.dtype, device=dev)
    nfb = torch.zeros(1, dtype=torch.int32, device=dev)
    m = {"quadric": 0, "mean": 1}[mode]

    def do_clusters():
        _lib.check(lib.dfh_mesh_simplify_clusters(v.data_ptr(), dtype_code(v), V, f.data_ptr(), F, cell, org, m, 1e-3, keys.data_ptr(), st["order"].data_ptr(),
                                                  st["corder"].data_ptr(), cbeg.data_ptr(), cend.data_ptr(), cstart.data_ptr(), ccount.data_ptr(), C,
                                                  cverts.data_ptr(), nfb.data_ptr(), ws.data_ptr(), wsb, S), "clusters")

    def do_attr():
        _lib.check(lib.dfh_mesh_simplify_attr(nrm.data_ptr(), dtype_code(nrm), V, 3, st["order"].data_ptr(), cstart.data_ptr(), ccount.data_ptr(), C,
                                              cn.data_ptr(), S), "attr")

    fout, fidx, cmap, kept, vmap = i32(F, 3), i32(F), i32(C), i32(C), i32(V)
    counts = (ctypes.c_long * 2)(0, 0)

    def do_faces():
        _lib.check(lib.dfh_mesh_simplify_faces(f.data_ptr(), V, F, vclus.data_ptr(), C, 1, fout.data_ptr(), fidx.data_ptr(), cmap.data_ptr(), kept.data_ptr(),
                                               vmap.data_ptr(), counts, ws.data_ptr(), wsb, S), "faces")

    out["clusters"] = timed(do_clusters)
    out["attr"] = timed(do_attr)
    out["faces"] = timed(do_faces)
    return out, C, int(nfb.item()), counts[0], counts[1]


def measure(name, T, level):
    mc = lambda: mesh.marching_cubes(T, level)
    v, f, nrm, _ = mc()
    V, F = v.shape[0], f.shape[0]
    say("%s: %d vertices, %d faces" % (name, V, F))
    say("  marching_cubes (same volume)         : %8.3f ms  (%.3f .. %.3f)" % timed(mc))
    say("  filter_components(min_faces=10)      : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.filter_components(v, f, nrm, min_faces=10)))
    for cell in (2.0, 4.0):
        st, C, nfb, nv, nf = stages(v, f, nrm, cell, "quadric")
        say("  cell %.0f: %d clusters, %d fell back; %d -> %d vertices, %d -> %d faces (%.1f x fewer)" % (cell, C, nfb, V, nv, F, nf, F / max(nf, 1)))
        total = sum(x[0] for x in st.values())
        for k in ("keys", "sorts", "group", "clusters", "attr", "faces"):
            say("    %-10s: %8.3f ms  (%.3f .. %.3f)  %4.1f %% of the stages" % (k, *st[k], 100.0 * st[k][0] / total))
        stm = stages(v, f, nrm, cell, "mean")[0]
        say("    clusters, mode mean (no quadrics): %8.3f ms  (%.3f .. %.3f)" % stm["clusters"])
        for mode in ("quadric", "mean"):
            whole = timed(lambda: mesh.simplify(v, f, nrm, cell=cell, mode=mode))
            sv, sf, sn, info = mesh.simplify(v, f, nrm, cell=cell, mode=mode)
            cmpd = mesh.compare_meshes(sv.cpu().numpy(), sf.cpu().numpy(), v.cpu().numpy(), f.cpu().numpy())
            say("    mesh.simplify, mode %-7s       : %8.3f ms  (%.3f .. %.3f); accuracy mean %.4f rms %.4f max %.4f, completeness mean %.4f rms %.4f max %.4f voxel"
                % (mode, *whole, cmpd["accuracy"]["mean"], cmpd["accuracy"]["rms"], cmpd["accuracy"]["max"], cmpd["completeness"]["mean"],
                   cmpd["completeness"]["rms"], cmpd["completeness"]["max"]))


say("K24 mesh simplification on %s, %d reps" % (torch.cuda.get_device_name(0), a.reps))
T3 = config3_volume()
measure("config 3 (256^3)", T3, 0.0)
del T3
torch.cuda.empty_cache()
if not a.no_512:
    measure("config 5 (512^3)", config5_volume(), 0.0)
if a.out:
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")
