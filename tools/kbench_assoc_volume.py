"""Times the volume data term's association (dfh_gn_associate_volume) against the stand-alone projective association it replaces
(dfh_gn_associate with 1 view and with all views), in one process, on the samples of bench.py's frame legs:

    config 3: 256^3, 512 nodes, 3 views of 640x480      config 5: 512^3, 2 048 nodes, 8 views of 1280x720

    python tools/kbench_assoc_volume.py [--res 256 512] [--out profiles/r7_assoc_volume.txt]

Each call is timed with HIP events: 5 warm-ups, then 20 calls, min and median in microseconds.  Requirement (the issue that added the
kernel): the volume association's MEDIAN is below the all-views association's MINIMUM at both sizes.  Reported only: the 1-view
ratio, and the frame time of SlabFrame.step(data_term="volume") against "depth" with its stage split (stage_ms: a synchronisation
after every stage, so the sums are not throughput).  Prints one JSON line per size; --out appends the same lines to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicfusion_body_amd import scene                      # noqa: E402
from dynamicfusion_body_amd.pipeline import SlabFrame         # noqa: E402

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])


def time_calls(fn, warm=5, n=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {"min_us": float(np.min(us)), "median_us": float(np.median(us))}


def run(R, frames_per_term=3):
    cam, N = ("C2", 512) if R <= 256 else ("C5", 2048)
    angles = (0.0, 40.0, -40.0) if R <= 256 else tuple(45.0 * v for v in range(8))
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=4.0, distributed=False)
    lws = [scene.view_extrinsic(a) for a in angles]
    for lw in lws:
        sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda(), lw)
    sf.refresh_samples()

    def depths(f):
        off = np.array([0.10, -0.07, 0.05]) * (f + 1) * scale
        return [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off,
                                                    sphere_r=scene.SPHERE_R * (1.0 + 0.004 * (f + 1)))).cuda() for lw in lws]
    ds = depths(0)
    sf.step(ds, lws, gn_iters=10)                           # frame 0: allocates, leaves a live volume and steady-state samples
    sv = sf.fs.solver
    band = float(torch.tensor(sf.tvox, dtype=sf.live.dtype))
    rec = {"res": R, "nodes": N, "views": len(lws), "samples": int(sv.S)}
    rec["volume"] = time_calls(lambda: sv.associate_volume(sf.live, IDENT, band, max_dist=2.0))
    rec["volume_valid"] = int(sv.valid.sum())
    rec["depth_1_view"] = time_calls(lambda: sv.associate_depth(ds[0], K, Kinv, lws[0], scale, center, R / 2, IDENT, max_dist=2.0))
    rec["depth_all_views"] = time_calls(lambda: sv.associate_depth(ds, K, Kinv, lws, scale, center, R / 2, IDENT, max_dist=2.0))
    rec["depth_all_views_valid"] = int(sv.valid.sum())
    rec["requirement_volume_median_below_all_views_min"] = bool(rec["volume"]["median_us"] < rec["depth_all_views"]["min_us"])
    rec["volume_median_over_1_view_min"] = rec["volume"]["median_us"] / rec["depth_1_view"]["min_us"]
    f = 1
    for term in ("depth", "volume", "depth", "volume"):     # (alternating: the first pair warms both paths up)
        stages = {}
        for _ in range(frames_per_term):
            sf.step(depths(f), lws, gn_iters=10, stage_ms=stages, data_term=term)
            f += 1
        rec["frame_ms_" + term] = {"total": sum(stages.values()) / frames_per_term,
                                   "stage_ms_with_syncs": {k: v / frames_per_term for k, v in stages.items()}}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ok = True
    for R in args.res:
        rec = run(R)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ok = ok and rec["requirement_volume_median_below_all_views_min"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
