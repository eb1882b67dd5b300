"""Times the depth data term with and without its normal-compatibility gate (dfh_gn_*_gated), in one process, on the samples of
bench.py's frame legs:

    config 3: 256^3, 512 nodes, 3 views of 640x480      config 5: 512^3, 2 048 nodes, 8 views of 1280x720

    python tools/kbench_normal_gate.py [--res 256 512] [--band 4] [--out profiles/r13_normal_gate.txt]

(a) one frame's solve -- 2 sampled rigid-mode steps (every 4th tile) + 10 node iterations from the same start field, HIP events
round the whole call sequence -- ungated and gated (min_cos 0.5) on the same cleaned maps and normal maps; (b) SlabFrame.step()
with a DepthPrep, without and with normal_gate=0.5, the legs on loops of their own that see the same frames.  The variants
ALTERNATE call by call, every variant is there twice (the difference of the twins is the spread): 3 warm-up rounds, then 20
rounds, min / quartiles / median.  Nothing is enforced: the gate is opt-in.  Prints one JSON line per size; --out appends it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dynamicfusion_body_amd import scene                      # noqa: E402
from dynamicfusion_body_amd.depth_prep import DepthPrep       # noqa: E402
from dynamicfusion_body_amd.pipeline import SlabFrame         # noqa: E402

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
MIN_COS = 0.5


def time_alternating(variants, warm=3, n=20):
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


def loop(R, band, normal_gate=None):
    cam, N = ("C2", 512) if R <= 256 else ("C5", 2048)
    angles = (0.0, 40.0, -40.0) if R <= 256 else tuple(45.0 * v for v in range(8))
    H, W, fx, cx, cy = scene.CAMERAS[cam]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=band, distributed=False,
                   depth_prep=DepthPrep(), normal_gate=normal_gate)
    lws = [scene.view_extrinsic(a) for a in angles]
    for lw in lws:
        sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda(), lw)
    sf.refresh_samples()
    return sf, K, scale, center, lws, (H, W)


def frames_of(K, scale, lws, size, n):
    out = []
    for f in range(n):
        off = np.array([0.10, -0.07, 0.05]) * ((f % 2) + 1) * scale
        out.append([torch.from_numpy(scene.render_depth(K, lw, size[0], size[1], dtype=np.float32, invalid_frac=0.0, sphere_offset=off,
                                                        sphere_r=scene.SPHERE_R * (1.0 + 0.004 * ((f % 2) + 1)))).cuda() for lw in lws])
    return out


def run(R, band):
    sf, K, scale, center, lws, size = loop(R, band)
    fr = frames_of(K, scale, lws, size, 2)
    sf.step(fr[0], lws, gn_iters=10)                        # frame 0: allocates, leaves steady-state samples and this frame's maps
    sv = sf.fs.solver
    Kinv = np.linalg.inv(K)
    ds, normals = sf.clean_depth, sf.live_normals
    rw, lm_abs, lm_rel, max_dist, huber = 5.0, 10.0, 1e-2, 2.0, 0.5          # SlabFrame.step's defaults
    start = sv.node_dq.clone()
    rec = {"res": R, "nodes": int(sv.N), "views": len(lws), "samples": int(sv.S), "band": band, "min_cos": MIN_COS,
           "what": "normal gate: frame solve and step() A/B, us"}

    def solve(gated):
        kw = {"normals": normals, "normal_cos": MIN_COS} if gated else {}

        def call():
            sv.node_dq.copy_(start)
            sv.global_sampled(ds, K, Kinv, lws, scale, center, R / 2, IDENT, max_dist, huber, 0.1, n_steps=2, stride=sf.GLOBAL_STRIDE, **kw)
            sv.iterate_associated(ds, K, Kinv, lws, scale, center, R / 2, IDENT, rw, max_dist, huber, lm_abs, lm_rel, n_iters=10, **kw)
        return call
    rec["solve"] = time_alternating({"ungated": solve(False), "gated": solve(True), "ungated_again": solve(False), "gated_again": solve(True)})
    for gated in (False, True):
        solve(gated)()
        rec["valid_after_solve_" + ("gated" if gated else "ungated")] = int(sv.valid.sum())
    # step(): four loops of their own on the same frames (a step changes its loop's state; the legs must not see each other's)
    legs = {"plain": None, "gated": MIN_COS, "plain_again": None, "gated_again": MIN_COS}
    loops = {}
    for name, gate in legs.items():
        l = loop(R, band, normal_gate=gate)[0]
        l.step(fr[0], lws, gn_iters=10)
        loops[name] = l
    state = {"f": 1}

    def stepper(l):
        def call():
            l.step(fr[state["f"] % 2], lws, gn_iters=10)
        return call
    variants = {name: stepper(l) for name, l in loops.items()}
    us = {name: [] for name in variants}
    for r in range(3 + 20):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 3:
                us[name].append(a.elapsed_time(b) * 1e3)
        state["f"] += 1
    q = lambda v, p: float(np.percentile(v, p))
    rec["step"] = {name: {"min_us": float(np.min(v)), "q1_us": q(v, 25), "median_us": q(v, 50), "q3_us": q(v, 75)} for name, v in us.items()}
    rec["step_samples"] = {name: int(l.fs.solver.S) for name, l in loops.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--band", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for R in args.res:
        line = json.dumps(run(R, args.band))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
