#!/usr/bin/env python3
"""K23, mesh connected components, timed by HIP events (medians of --reps runs after a warm-up run; each line's spread against
itself is printed as min .. max) on
  config 3 : the marching-cubes mesh of the config-3 scene (256^3, 3 views of camera C2)
  config 5 : the marching-cubes mesh of the config-5 scene (512^3, the 8-view orbit of camera C5)
  fragments: the config-3 mesh with 10 000 single triangles added (10 001 or more components)
per mesh: the labelling call (dfh_mesh_components: it synchronises, so the events bracket a host wait too), the table, the
compaction (keep: the components of at least 10 faces), the whole mesh.filter_components(min_faces=10) with one attribute, and
beside them marching_cubes on the same volume in the same run, the numpy restatement (tests/components_np.py) on the host, once,
and the labelling pass's byte floor, 12 F + 4 V read and 4 V written, at --floor-gbs (default 4000 GB/s, half of the 8 TB/s line:
what a short read-mostly pass reaches; the conclusion does not hang on the factor of two).
usage: python tools/kbench_components.py [--reps 50] [--no-512] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from dynamicfusion_body_amd import FusionDM, _lib, mesh, scene
from dynamicfusion_body_amd.device import current_stream_ptr, dtype_code
from dynamicfusion_body_amd.pipeline import SlabFrame

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--no-512", action="store_true")
ap.add_argument("--floor-gbs", type=float, default=4000.0)
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


def config3_volume(R=256):
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


def with_fragments(v, f, n=10000, seed=0):
    rng = np.random.default_rng(seed)
    lo, hi = v.min(dim=0).values.cpu().numpy(), v.max(dim=0).values.cpu().numpy()
    c = rng.uniform(lo, hi, size=(n, 1, 3))
    tri = torch.from_numpy((c + rng.uniform(-0.5, 0.5, size=(n, 3, 3))).reshape(-1, 3).astype(np.float32)).cuda()
    tf = torch.arange(3 * n, dtype=torch.int32, device="cuda").reshape(-1, 3) + v.shape[0]
    # interleave the fragments' faces with the mesh's (every k-th face), as fragments of a real volume lie among its cubes
    F = f.shape[0] + n
    at = torch.linspace(0, F - 1, n, device="cuda").long()
    is_frag = torch.zeros(F, dtype=torch.bool, device="cuda")
    is_frag[at] = True
    faces = torch.empty((F, 3), dtype=torch.int32, device="cuda")
    faces[is_frag] = tf[: int(is_frag.sum())]
    faces[~is_frag] = f[: F - int(is_frag.sum())]
    return torch.cat([v, tri]).contiguous(), faces.contiguous()


def measure(name, v, f, nrm, mc):
    lib = _lib.load()
    V, F = v.shape[0], f.shape[0]
    say("%s: %d vertices, %d faces" % (name, V, F))
    if mc is not None:
        say("  marching_cubes (same volume)   : %8.3f ms  (%.3f .. %.3f)" % timed(mc))
    comps = mesh.connected_components(v, f)
    C = comps.n
    keep = mesh.keep_mask(comps, min_faces=10)
    say("  %d components, %d of at least 10 faces; largest %d faces" % (C, int(keep.sum()), int(comps.n_faces.max())))
    ws = mesh._components_workspace(lib, V, F, v.device)
    root, vc, fc = torch.empty_like(comps.vert_root), torch.empty_like(comps.vert_comp), torch.empty_like(comps.face_comp)
    n = ctypes.c_long(0)

    def label():
        _lib.check(lib.dfh_mesh_components(f.data_ptr(), V, F, root.data_ptr(), vc.data_ptr(), fc.data_ptr(), ctypes.byref(n), ws.data_ptr(),
                                           ws.numel() * 8, current_stream_ptr()), "dfh_mesh_components")

    out = [torch.empty_like(getattr(comps, k)) for k in ("root", "n_verts", "n_faces", "bbox_min", "bbox_max", "area")]

    def table():
        _lib.check(lib.dfh_mesh_component_table(v.data_ptr(), dtype_code(v), V, f.data_ptr(), F, root.data_ptr(), vc.data_ptr(), fc.data_ptr(), C,
                                                *[t.data_ptr() for t in out], ws.data_ptr(), ws.numel() * 8, current_stream_ptr()),
                   "dfh_mesh_component_table")

    ms = timed(label)
    floor_bytes = 12 * F + 4 * V + 4 * V
    say("  labelling                      : %8.3f ms  (%.3f .. %.3f); byte floor %.1f MB = %.4f ms at %.0f GB/s: %.0f x the floor"
        % (ms + (floor_bytes / 1e6, floor_bytes / a.floor_gbs / 1e6, a.floor_gbs, ms[0] / (floor_bytes / a.floor_gbs / 1e6))))
    assert n.value == C and torch.equal(vc, comps.vert_comp) and torch.equal(fc, comps.face_comp)
    say("  table                          : %8.3f ms  (%.3f .. %.3f)" % timed(table))
    assert torch.equal(out[5].view(torch.int64), comps.area.view(torch.int64)) and torch.equal(out[2], comps.n_faces)
    say("  compaction                     : %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.compact_components(comps, keep)))
    say("  filter_components(min_faces=10): %8.3f ms  (%.3f .. %.3f)" % timed(lambda: mesh.filter_components(v, f, nrm, min_faces=10)))
    import components_np as CN
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    t0 = time.perf_counter()
    want = CN.components(vn, fn)
    t1 = time.perf_counter()
    CN.compact(fn, want["vert_comp"], want["face_comp"], CN.keep_mask(want, min_faces=10), True)
    t2 = time.perf_counter()
    same = (np.array_equal(want["vert_comp"], comps.vert_comp.cpu().numpy()) and np.array_equal(want["n_faces"], comps.n_faces.cpu().numpy())
            and np.array_equal(want["area"].view(np.uint64), comps.area.cpu().numpy().view(np.uint64)))
    say("  numpy restatement on the host  : %8.1f ms labels + table, %.1f ms compaction (one run); equal to the device: %s"
        % (1e3 * (t1 - t0), 1e3 * (t2 - t1), same))


say("K23 mesh connected components on %s, %d reps" % (torch.cuda.get_device_name(0), a.reps))
T3 = config3_volume()
v3, f3, n3, _ = mesh.marching_cubes(T3, 0.0)
measure("config 3 (256^3)", v3, f3, n3, lambda: mesh.marching_cubes(T3, 0.0))
vf, ff = with_fragments(v3, f3)
measure("config 3 + 10 000 fragments", vf, ff, torch.cat([n3, torch.zeros((30000, 3), dtype=n3.dtype, device="cuda")]), None)
del T3, v3, f3, n3, vf, ff
torch.cuda.empty_cache()
if not a.no_512:
    T5 = config5_volume()
    v5, f5, n5, _ = mesh.marching_cubes(T5, 0.0)
    measure("config 5 (512^3)", v5, f5, n5, lambda: mesh.marching_cubes(T5, 0.0))
if a.out:
    with open(a.out, "w") as fp:
        fp.write("\n".join(lines) + "\n")
