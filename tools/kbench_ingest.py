"""HIP-event timings of the RGB-D ingest (K19, csrc/dfh_ingest.hip).

  1. the stage alone on a rig of 8 views: 640 x 480 depth with 1280 x 720 colour (bilinear), 1280 x 720 both (bilinear and
     nearest), and depth only; beside each, the call's byte floor and the fraction of the measured HBM copy rate it reaches;
  2. for context, dfh_depth_prep (DepthPrep's defaults) on the stage's output maps of the same sizes;
  3. one frame of the composed loop (pipeline.SlabFrame.step) at config 3 (256^3, 512 nodes, 3 views of C2) and -- unless
     --no-512 -- config 5 (512^3, 2 048 nodes, 8 views of 1280 x 720) without the stage (float depth maps in) and with it (raw
     uint16 maps in), depth only and with colours fused (both loops then have a colour volume; colour the size of depth).

The byte floor of a call with colour: 2 B read and 12 B written per depth pixel (depth, colour, colour-only depth), 8 B per colour
pixel for the z-buffer (the clear's store and one read or atomic), and the colour image read once (C bytes per colour pixel).
Depth only: 2 B read and 4 B written per depth pixel.  Variants alternate inside a round, medians of --reps per round, two rounds.

    python tools/kbench_ingest.py [--reps 30] [--no-512] [--stage-only] [--out profiles/r19_ingest.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29          # float4 copy rate measured on the MI355X (8.0 TB/s specified)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-512", action="store_true")
    ap.add_argument("--stage-only", action="store_true", help="section 1 only (for a kernel trace of the stage's three launches)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from dynamicfusion_body_amd import scene
    from dynamicfusion_body_amd.depth_prep import DepthPrep
    from dynamicfusion_body_amd.ingest import RGBDCalibration, RGBDIngest
    from dynamicfusion_body_amd.pipeline import SlabFrame

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3                                      # us

    def rounds(variants, reps):
        """variants: {name: fn}; two rounds, inside a round the variants alternate repetition by repetition."""
        out = {name: [] for name in variants}
        for _ in range(2):
            acc = {name: [] for name in variants}
            for fn in variants.values():                                    # warm-up
                fn()
            for _ in range(reps):
                for name, fn in variants.items():
                    acc[name].append(timed(fn))
            for name in variants:
                out[name].append(float(np.median(acc[name])))
        return out

    rng = np.random.default_rng(19)
    V = 8

    def rig(depth_size, color_size, sample):
        """8 views: a slanted scene with steps around 1-3 m, mild distortion on both cameras, a 5 cm baseline."""
        Hd, Wd = depth_size
        Hc, Wc = color_size
        f = 0.9 * Wd
        jj, ii = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
        raws, imgs, cal = [], [], []
        for v in range(V):
            base = 1500 + 400 * np.sin(ii / 70.0 + v) + 300 * np.cos(jj / 50.0)
            base = np.where((ii // 60 + jj // 50 + v) % 4 == 0, base + 900, base)
            raw = np.rint(base + rng.integers(-3, 4, size=base.shape)).astype(np.uint16)
            raw[rng.random(base.shape) < 0.02] = 0
            raws.append(torch.from_numpy(raw.view(np.int16)).cuda())
            imgs.append(torch.from_numpy(rng.integers(0, 256, size=(Hc, Wc, 4), dtype=np.uint8)).cuda())
            r = Wc / float(Wd)
            T = np.hstack([np.eye(3), np.array([[-0.05], [0.0], [0.0]])])
            cal.append(RGBDCalibration((f * 1.01, f * 0.99, (Wd - 1) / 2.0 + 0.3, (Hd - 1) / 2.0 - 0.2), (0.1, -0.05, 1e-3, -1e-3, 0.01),
                                       (f * r, f * r, (Wc - 1) / 2.0, (Hc - 1) / 2.0), (-0.08, 0.03, -5e-4, 7e-4, -0.005), T))
        ing = RGBDIngest(cal, depth_size, color_size, (f, f, (Wd - 1) / 2.0, (Hd - 1) / 2.0), sample=sample, max_splat=8)
        return ing, raws, imgs

    say("RGB-D ingest, %d views per call; %d repetitions per round, two rounds; floor = bytes / %.2f TB/s" % (V, args.reps, HBM_COPY_TBS))
    say()
    say("1. the stage alone (us, median per round | round 2; byte floor; fraction of the floor's rate reached in round 2)")
    prep_inputs = {}
    for name, dsz, csz, sample, colour in (("640x480 depth, 1280x720 colour, bilinear", (480, 640), (720, 1280), "bilinear", True),
                                           ("1280x720 both, bilinear", (720, 1280), (720, 1280), "bilinear", True),
                                           ("1280x720 both, nearest", (720, 1280), (720, 1280), "nearest", True),
                                           ("1280x720 depth only", (720, 1280), (720, 1280), "bilinear", False),
                                           ("640x480 depth only", (480, 640), (720, 1280), "bilinear", False)):
        ing, raws, imgs = rig(dsz, csz, sample)
        nd, nc = V * dsz[0] * dsz[1], V * csz[0] * csz[1]
        out = ing(raws, imgs if colour else None)
        torch.cuda.synchronize()
        bufs = out if colour else (out[0], None, None)

        def call(ing=ing, raws=raws, imgs=imgs if colour else None, bufs=bufs):
            ing(raws, imgs, out=bufs)
        r = rounds({"a": call, "b": call}, args.reps)
        floor_b = (14 * nd + 12 * nc) if colour else 6 * nd
        floor_us = floor_b / (HBM_COPY_TBS * 1e6)
        best = min(r["a"][1], r["b"][1])
        valid = float((out[0] != 0).float().mean())
        has = float((out[2] != 0).float().mean()) if colour else float("nan")
        say("    %-42s %8.1f | %8.1f   (b) %8.1f | %8.1f   floor %6.1f MB = %6.1f us   %4.1f %%   valid %.3f coloured %.3f"
            % (name, r["a"][0], r["a"][1], r["b"][0], r["b"][1], floor_b / 1e6, floor_us, 100.0 * floor_us / best, valid, has))
        if not colour:
            prep_inputs[name] = (ing, [out[0][v].clone() for v in range(V)])
    if args.stage_only:
        return
    say()
    say("2. for context: dfh_depth_prep (radius 3, normals and mask) on the stage's output maps (us, median per round | round 2)")
    for name, (ing, maps) in prep_inputs.items():
        p = DepthPrep()
        res = p(maps, ing.Kinv)
        torch.cuda.synchronize()
        bufs = (torch.stack(res[0]), res[1])

        def call(p=p, maps=maps, ing=ing, bufs=bufs):
            p(maps, ing.Kinv, out=bufs)
        r = rounds({"a": call}, args.reps)
        say("    %-42s %8.1f | %8.1f" % (name.replace(" depth only", ""), r["a"][0], r["a"][1]))

    def loop(R, N, cam, angles, ingest, colour):
        H, W, fx, cx, cy = scene.CAMERAS[cam]
        K = scene.intrinsics(fx, cx, cy)
        scale, center, tdist = scene.grid_params(R)
        node_pos, node_w = scene.fibonacci_nodes(N, R)
        lws = [scene.view_extrinsic(a) for a in angles]
        ing = None
        if ingest:
            k4 = (fx, fx, cx, cy)
            ing = RGBDIngest([RGBDCalibration(k4, None, k4, None, np.hstack([np.eye(3), [[-0.03], [0.0], [0.0]]])) for _ in lws],
                             (H, W), (H, W), k4)
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=4.0, distributed=False,
                       color_band=1.5 if colour else None, ingest=ing)
        first = [scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0) for lw in lws]
        if ingest:
            sf.integrate([np.rint(-d.astype(np.float64) / 1e-3).astype(np.uint16) for d in first], lws)
        else:
            for d, lw in zip(first, lws):
                sf.integrate(torch.from_numpy(d).cuda(), lw)
        sf.refresh_samples()
        frames = []
        for f in range(4):
            off = np.array([0.10, -0.07, 0.05]) * (f + 1) * scale
            ds = [scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off) for lw in lws]
            if ingest:
                ds = [torch.from_numpy(np.rint(-d.astype(np.float64) / 1e-3).astype(np.uint16).view(np.int16)).cuda() for d in ds]
            else:
                ds = [torch.from_numpy(d).cuda() for d in ds]
            frames.append(ds)
        cols = [torch.from_numpy(rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)).cuda() for _ in lws] if colour else None
        state = {"f": 0}

        def step():
            sf.step(frames[state["f"] % 4], lws, gn_iters=10, colors=cols)
            state["f"] += 1
        return step

    say()
    say("3. one frame of SlabFrame.step, 10 GN iterations (us, median per round | round 2)")
    configs = [("config 3: 256^3, 512 nodes, 3 views of C2", 256, 512, "C2", (0.0, 40.0, -40.0))]
    if not args.no_512:
        configs.append(("config 5: 512^3, 2 048 nodes, 8 views of C5", 512, 2048, "C5", tuple(45.0 * v for v in range(8))))
    for title, R, N, cam, angles in configs:
        say("  %s" % title)
        for colour in (False, True):
            variants = {"float maps in%s" % (", colours" if colour else ""): loop(R, N, cam, angles, False, colour),
                        "raw maps in, ingest%s" % (", colours" if colour else ""): loop(R, N, cam, angles, True, colour)}
            r = rounds(variants, max(4, args.reps // 3))
            for name, v in r.items():
                say("    %-34s %10.1f | %10.1f" % (name, v[0], v[1]))
            del variants
            torch.cuda.empty_cache()
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
