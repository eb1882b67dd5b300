"""One line per (class, method, case) with the SHA-256 of what the public methods of Fusion / FusionDM return or write, on a
16^3 volume: the check that a change behind the two classes moved no bit.  Run it once with the package of either commit on
PYTHONPATH (the compiled library may be shared through DFH_LIB_PATH) and compare the two outputs line by line.

    python tools/facade_digest.py > head.txt
    PYTHONPATH=<a checkout of the other commit> python tools/facade_digest.py > other.txt
"""
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

import dynamicfusion_body_amd
from dynamicfusion_body_amd import Fusion, FusionDM, scene

R, H, W = 16, 24, 32
SCALE, CENTER, TDIST = scene.grid_params(R)                    # 0.1 m voxels around the scene's sphere: its radius is 5 voxels
K = scene.intrinsics(30.03113, 15.97033, 11.96003)             # camera C1 at a tenth of its resolution
LWS = [scene.view_extrinsic(a) for a in (0.0, 40.0)]


def volume():
    """A sphere of radius 5 voxels (negative inside, truncated at +-TDIST) and a detached blob of two voxels."""
    i = np.arange(R) - (R - 1) / 2.0
    r = np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    T = np.clip((r - 5.0) * SCALE, -TDIST, TDIST)
    T[1, 1, 1:3] = -0.5 * TDIST
    return T.astype(np.float32)


def depth_maps(dtype=np.float32):
    return [scene.render_depth(K, lw, H, W, dtype=dtype, wall_z=None) for lw in LWS]


def images():
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in LWS]


def digest(x):
    h = hashlib.sha256()

    def feed(a):
        if a is None:
            h.update(b"None")
        elif isinstance(a, (tuple, list)):
            h.update(b"seq%d" % len(a))
            for b in a:
                feed(b)
        elif isinstance(a, (int, float, np.integer, np.floating)):
            h.update(repr(float(a)).encode())
        else:
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            h.update(("%s%s" % (a.dtype, a.shape)).encode())
            h.update(np.ascontiguousarray(a).tobytes())
    feed(x)
    return h.hexdigest()


def file_digest(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def say(cls, method, case, d):
    print("%-9s %-26s %-22s %s" % (cls, method, case, d), flush=True)


def stored_mesh(o):
    return (o._vertices, getattr(o, "_faces", None), o._normals)


def nodes_of(o):
    return [(int(n[0]), np.asarray(n[1]), np.asarray(n[2]), float(n[3])) for n in o._nodes]


def shared(name, o, tmp):
    """The methods both classes have, on an object whose canonical volume is volume() with unit weights and whose graph is built."""
    live = np.roll(volume(), 1, axis=0)
    o.marching_cubes()
    say(name, "marching_cubes", "stored", digest(stored_mesh(o)))
    o.min_component_faces = 20
    o.marching_cubes()
    say(name, "marching_cubes", "min_component_faces", digest(stored_mesh(o)))
    o.min_component_faces = None
    say(name, "marching_cubes", "tsdf", digest(o.marching_cubes(live)))
    say(name, "marching_cubes", "tsdf tensor step 2", digest(o.marching_cubes(torch.from_numpy(live).cuda(), step_size=2)))
    o.surface_samples(band=SCALE)
    say(name, "surface_samples", "stored", digest(stored_mesh(o)))
    say(name, "surface_samples", "tsdf", digest(o.surface_samples(live, band=1.5 * SCALE)))
    o.marching_cubes()
    for case in ("plain", "simplified", "coloured", "coloured simplified"):
        o.simplify_cell = 2.0 if "simplified" in case else None
        o._C = color_volume(o) if "coloured" in case else None
        o.write_canonical_mesh(tmp, "canonical.obj")
        say(name, "write_canonical_mesh", case, file_digest(os.path.join(tmp, "canonical.obj")))
    o.simplify_cell = None
    say(name, "live_frame_mesh", "own nodes", digest(o.live_frame_mesh()))
    say(name, "live_frame_mesh", "no nodes", digest(o.live_frame_mesh([])))
    wf = o.write_warp_field(tmp, "field")
    say(name, "write_live_frame_mesh", "own nodes", file_digest(o.write_live_frame_mesh(tmp, "live.obj", None)))
    say(name, "write_live_frame_mesh", "warp field file", file_digest(o.write_live_frame_mesh(tmp, "live2.obj", wf)))
    render = o.render_model if name == "FusionDM" else o.render_canonical
    r = render(LWS, H, W, K=K, scale=SCALE, center=CENTER)
    say(name, render.__name__, "coloured", digest((r.depth, r.normals, r.color)))
    o._C = None
    r = render(LWS[1], H, W, K=K, scale=SCALE, center=CENTER)
    say(name, render.__name__, "one view", digest((r.depth, r.normals)))
    say(name, "render_live_frame", "two views", digest(o.render_live_frame(LWS, H, W, K=K, scale=SCALE, center=CENTER)))
    for dt in (np.float32, np.float64):
        T, Wt = np.full((R, R, R), TDIST), np.zeros((R, R, R))
        for d, lw in zip(depth_maps(dt), LWS):
            out = o.fuseDepths(d, lw, T, Wt, scale=SCALE, center=CENTER)
        say(name, "fuseDepths", "numpy %s" % np.dtype(dt).name, digest(out))
        T, Wt = torch.full((R, R, R), TDIST, device="cuda"), torch.zeros((R, R, R), device="cuda")
        for d, lw in zip(depth_maps(dt), LWS):
            out = o.fuseDepths(torch.from_numpy(d).cuda(), lw, T, Wt, scale=SCALE, center=CENTER, wmax=1.0)
        say(name, "fuseDepths", "tensor %s" % np.dtype(dt).name, digest(out))
    say(name, "update_graph", "n_new", digest(o.update_graph()))
    say(name, "update_graph", "nodes", digest(nodes_of(o) + [o._neighbor_look_up]))
    o.updateTSDF(live)
    say(name, "updateTSDF", "rolled volume", digest(o.tsdf_device))
    say(name, "_tsdf / _tsdfw", "getters", digest((o._tsdf, o._tsdfw)))


def color_volume(o):
    from dynamicfusion_body_amd import kernels
    C = kernels.color_volume((R, R, R))
    kernels.integrate_color(C, o._T, o._Wt, [torch.from_numpy(d).cuda() for d in depth_maps()], images(), K, np.linalg.inv(K),
                            LWS, SCALE, CENTER, TDIST, 1.5 * SCALE)
    return C


def main():
    print("# package: %s" % os.path.dirname(os.path.abspath(dynamicfusion_body_amd.__file__)), file=sys.stderr)
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        f = Fusion(volume(), TDIST, subsample_rate=3.0, marching_cubes_step_size=1, write_warpfield=False)
        f.InitializeCanonicalSpace(tsdf=volume(), K=K)
        f._tsdfw = np.ones((R, R, R))
        say("Fusion", "InitializeCanonicalSpace", "tsdf", digest(nodes_of(f) + [f._neighbor_look_up]))
        shared("Fusion", f, tmp)
        f.updateTSDF_depths(depth_maps(), LWS, scale=SCALE, center=CENTER, colors=images())
        say("Fusion", "updateTSDF_depths", "coloured", digest((f._T, f._Wt, f._C)))
        f.updateTSDF_depths(depth_maps(np.float64), LWS, weight="unit", scale=SCALE, center=CENTER)
        say("Fusion", "updateTSDF_depths", "float64 maps, unit", digest((f._T, f._Wt, f._C)))
        for case, colors in (("depths", None), ("depths coloured", images())):
            f = Fusion(volume(), TDIST, subsample_rate=3.0, marching_cubes_step_size=1, write_warpfield=False)
            f.InitializeCanonicalSpace(depths=depth_maps(), lws=LWS, K=K, tsdf_size=R, scale=SCALE, center=CENTER, colors=colors)
            say("Fusion", "InitializeCanonicalSpace", case, digest((f._T, f._Wt, f._C, stored_mesh(f), nodes_of(f))))

        g = FusionDM(TDIST, K, tsdf_res=R, subsample_rate=3.0, marching_cubes_step_size=1, write_warpfield=False)
        g._tsdf, g._tsdfw = volume(), np.ones((R, R, R))
        g.marching_cubes()
        g._radius = 2.0
        g.construct_graph()
        say("FusionDM", "construct_graph", "radius 2", digest(nodes_of(g) + [g._neighbor_look_up]))
        shared("FusionDM", g, tmp)
        for case, colors in (("plain", None), ("coloured", images())):
            g = FusionDM(TDIST, K, tsdf_res=R)
            out = g.compute_live_tsdf(depth_maps(), LWS, UseAutoAlignment=True, colors=colors)
            say("FusionDM", "compute_live_tsdf", case, digest((out, g._C, g._IND)))
        g = FusionDM(TDIST, K, tsdf_res=R)
        out = g.compute_live_tsdf([depth_maps()[0], depth_maps(np.float64)[1] * (1 + 1e-12)], LWS, as_numpy=False)
        say("FusionDM", "compute_live_tsdf", "mixed dtypes, tensors", digest(out))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
