"""Times the volume data term's association (dfh_gn_associate_volume) against the stand-alone projective association it replaces
(dfh_gn_associate with 1 view and with all views), in one process, on the samples of bench.py's frame legs:

    config 3: 256^3, 512 nodes, 3 views of 640x480      config 5: 512^3, 2 048 nodes, 8 views of 1280x720

    python tools/kbench_assoc_volume.py [--res 256 512] [--out profiles/r7_assoc_volume.txt]

Each call is timed with HIP events: 5 warm-ups, then 20 calls, min and median in microseconds.  Requirement (the issue that added the
kernel): the volume association's MEDIAN is below the all-views association's MINIMUM at both sizes.  Reported only: the 1-view
ratio, and the frame time of SlabFrame.step(data_term="volume") against "depth" with its stage split (stage_ms: a synchronisation
after every stage, so the sums are not throughput).  Prints one JSON line per size; --out appends the same lines to a file.

    python tools/kbench_assoc_volume.py --fused [--res 256 512] [--out profiles/r8_volume_fused.txt]

--fused times the layers that put the volume term's association inside the build instead: one frame's solve (2 rigid-mode steps +
10 node iterations from the same start field, HIP events around the whole call sequence, so host gaps that starve the device
count) through (a) iterate_volume as built, (b) the same under py_gn_no_fused_assoc=1 -- the launch sequence of the commit before
the fused build, kept alive by the option -- (b2) the same variant again, whose difference to (b) is the spread, and (c)
iterate_associated with all views; (d) the two rigid-mode steps, sampled against built.  The variants ALTERNATE call by call: 3
warm-up rounds, then 25 rounds, min / median / quartiles in microseconds.  Then the SlabFrame.step stage split for
data_term="volume" (default, and global_built=False) and "depth": the three legs alternate frame by frame, medians of 7 frames
each (stage_ms: a synchronisation after every stage and the plan build inside "solve", so these are not throughput).  Expectation, reported as booleans, not enforced: (a) beats (b)
by more than |median(b) - median(b2)|, and the sampled step beats the built one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicfusion_body_amd import _lib, scene                # noqa: E402
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


def time_alternating(variants, warm=3, n=25):
    """variants: name -> callable; one call of each per round, in turn.  Returns name -> {min, q1, median, q3} in us."""
    us = {name: [] for name in variants}
    for r in range(warm + n):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warm:
                us[name].append(a.elapsed_time(b) * 1e3)
    q = lambda v, p: float(np.percentile(v, p))
    return {name: {"min_us": float(np.min(v)), "q1_us": q(v, 25), "median_us": q(v, 50), "q3_us": q(v, 75)} for name, v in us.items()}


def steady_frame(R):
    """The bench's frame leg at R after one frame: (SlabFrame, K, Kinv, scale, center, views' extrinsics, depths(f))."""
    cam, N = ("C2", 512) if R <= 256 else ("C5", 2048)
    angles = (0.0, 40.0, -40.0) if R <= 256 else tuple(45.0 * v for v in range(8))
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
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
    sf.step(depths(0), lws, gn_iters=10)                    # frame 0: allocates, leaves a live volume and steady-state samples
    return sf, K, np.linalg.inv(K), scale, center, lws, depths


def run_fused(R, frames_per_term=7):
    sf, K, Kinv, scale, center, lws, depths = steady_frame(R)
    sv = sf.fs.solver
    ds = depths(0)
    band = float(torch.tensor(sf.tvox, dtype=sf.live.dtype))
    rw, lm_abs, lm_rel, max_dist, huber = 5.0, 10.0, 1e-2, 2.0, 0.5          # SlabFrame.step's defaults
    start = sv.node_dq.clone()
    rec = {"res": R, "nodes": int(sv.N), "views": len(lws), "samples": int(sv.S), "what": "fused volume term: frame solve A/B, us"}

    def with_option(option, fn):
        def call():
            _lib.set_option("py_gn_no_fused_assoc", 1 if option else None)    # (host side, outside the events)
            sv.node_dq.copy_(start)
            fn()
        return call
    vol = lambda ni, ng: sv.iterate_volume(sf.live, IDENT, rw, band, max_dist, huber, lm_abs, lm_rel, n_iters=ni, n_global=ng, global_lm=0.1)
    dep = lambda: sv.iterate_associated(ds, K, Kinv, lws, scale, center, R / 2, IDENT, rw, max_dist, huber, lm_abs, lm_rel, n_iters=10,
                                        n_global=2, global_lm=0.1)
    sampled = lambda stride: sv.global_sampled_volume(sf.live, IDENT, band, max_dist, huber, 0.1, n_steps=2, stride=stride)
    t = time_alternating({
        "a_solve_fused": with_option(False, lambda: vol(10, 2)),
        "b_solve_separate_assoc": with_option(True, lambda: vol(10, 2)),
        "b2_solve_separate_assoc_again": with_option(True, lambda: vol(10, 2)),
        "c_solve_depth_all_views": with_option(False, dep),
        "d_rigid_2_steps_sampled_stride_4": with_option(False, lambda: sampled(sf.GLOBAL_STRIDE)),
        "d_rigid_2_steps_sampled_stride_1": with_option(False, lambda: sampled(1)),
        "d_rigid_2_steps_built_fused": with_option(False, lambda: vol(0, 2)),
        "d_rigid_2_steps_built_separate_assoc": with_option(True, lambda: vol(0, 2)),
    })
    _lib.set_option("py_gn_no_fused_assoc", None)
    sv.node_dq.copy_(start)
    rec.update(t)
    a, b, b2 = (t[k]["median_us"] for k in ("a_solve_fused", "b_solve_separate_assoc", "b2_solve_separate_assoc_again"))
    rec["spread_b_us"] = abs(b - b2)
    rec["gain_a_over_b_us"] = min(b, b2) - a
    rec["expect_a_beats_b_by_more_than_spread"] = bool(min(b, b2) - a > abs(b - b2))
    rec["expect_sampled_beats_built"] = bool(t["d_rigid_2_steps_sampled_stride_4"]["median_us"] < t["d_rigid_2_steps_built_fused"]["median_us"])
    rec["volume_frame_solve_beats_depth"] = bool(a < t["c_solve_depth_all_views"]["median_us"])
    f = 1
    legs = (("depth", {}), ("volume", {}), ("volume_sampled_rigid", {"global_built": False}))
    per_frame = {name: [] for name, _ in legs}
    for r in range(1 + frames_per_term):                    # (the legs alternate frame by frame; the first round warms every path up)
        for name, kw in legs:
            stages = {}
            sf.step(depths(f), lws, gn_iters=10, stage_ms=stages, data_term=name.split("_")[0], **kw)
            f += 1
            if r > 0:
                per_frame[name].append(stages)
    for name, frames in per_frame.items():
        rec["frame_ms_" + name] = {"median_total": float(np.median([sum(st.values()) for st in frames])),
                                   "median_stage_ms_with_syncs": {k: float(np.median([st[k] for st in frames])) for k in frames[0]}}
    return rec


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
    ap.add_argument("--fused", action="store_true", help="the fused build / one-call solve / sampled rigid step A/B (reported, not enforced)")
    args = ap.parse_args()
    ok = True
    for R in args.res:
        rec = run_fused(R) if args.fused else run(R)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        ok = ok and rec.get("requirement_volume_median_below_all_views_min", True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
