"""HIP-event timings of the photometric term (K18, csrc/dfh_photometric.hip) on the bench's config-3 frame (256^3, 512 nodes, knn 4)
with three views.

  1. dfh_gn_add_photometric (rows kernel + accumulating gather) on the frame's own samples beside the same frame's fused build
     (dfh_gn_build with the three-view frame): the term alone, the build alone, build + term;
  2. one frame's solve (10 GN iterations, one library call) without and with the term;
  3. --parent-lib PATH: the one-call solve WITHOUT the term through this build's library and through the parent commit's
     (a second CDLL on the same problem structs): node DQs compared bit for bit, times beside the spread of each variant timed twice;
     then dfh_gn_add_photometric through both: the term's live scratch rows, tile-cost pairs and live flags, the system after
     build + term, active_out, view_out and resid_out compared bit for bit, and the term alone timed through both (this build's
     median of its four medians against the parent's largest).

The reference intensities are the luma of the first view's image at each sample's own projection plus noise, so residuals are tens
of intensity units and the Huber branch is taken by some rows.  Variants alternate inside a round, medians of --reps (default 30)
per round, every variant is timed in two rounds.

    python tools/kbench_photometric.py [--reps 30] [--parent-lib build_variants/parent/libdfusion_hip.so] [--out profiles/r18_photometric.txt]
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from dynamicfusion_body_amd import _lib, kernels, scene
    from dynamicfusion_body_amd.device import current_stream_ptr
    from dynamicfusion_body_amd.pipeline import FrameSolver

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    R, N, k = args.res, args.nodes, 4
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    T = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    Wt = torch.zeros_like(T)
    angles = (0.0, 40.0, -40.0)
    for a in angles:
        lw = scene.view_extrinsic(a)
        d = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
        kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    ident = torch.from_numpy(np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (N, 1))).cuda()
    fs = FrameSolver(K, scale, center, R / 2, knn=k, pcg_iters=10, distributed=False)
    fs.set_graph(node_pos, ident, node_w)
    S = fs.set_canonical(T, Wt, band=4.0)
    sv = fs.solver
    lws = [scene.view_extrinsic(a) for a in angles]
    off = np.array([0.6, -0.4, 0.3])
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, sphere_offset=off * scale,
                                                  sphere_r=scene.SPHERE_R * 1.02)).cuda() for lw in lws]
    rng = np.random.default_rng(18)
    # smooth images (a low-resolution pattern, upsampled): gradients of a few intensity units per pixel, as a camera's are
    colors = []
    for _ in lws:
        small = torch.from_numpy(rng.uniform(40.0, 215.0, size=(1, 3, H // 16 + 2, W // 16 + 2)))
        img = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
        colors.append(torch.cat([img.round().to(torch.uint8), torch.zeros((H, W, 1), dtype=torch.uint8)], dim=2).contiguous().cuda())
    kw = dict(rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.5)
    say("photometric term on the config-3 frame: %d^3, %d nodes, knn %d, %d samples, %d views of %d x %d; %d repetitions per round, two rounds"
        % (R, N, k, S, len(lws), W, H, args.reps))

    def timed(fn, reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]                    # us

    def rounds(variants, reps, prep=None):
        """variants: {name: fn}; two rounds, inside a round the variants alternate repetition by repetition."""
        out = {name: [] for name in variants}
        for rnd in range(2):
            acc = {name: [] for name in variants}
            for name, fn in variants.items():                               # warm-up
                if prep:
                    prep()
                fn()
            for _ in range(reps):
                for name, fn in variants.items():
                    if prep:
                        prep()
                    acc[name] += timed(fn, 1)
            for name in variants:
                out[name].append(float(np.median(acc[name])))
        return out

    def reset():
        sv.node_dq.copy_(ident)

    frame_args = (depths, fs.K, fs.Kinv, lws, fs.scale, fs.center, fs.half, fs.lw)
    band_sd = 2.0 * abs(scale)
    # references: the first build's own intensities plus noise (ref = 128 first: the residuals then give back I)
    fs.set_photometric(torch.full((S,), 128.0, dtype=torch.float64, device="cuda"), weight=1e-3, huber=10.0, band_sd=band_sd, presorted=True)
    sv.build_associated(*frame_args, kw["rw"], kw["max_dist"], kw["huber"], colors=colors)
    I0 = sv._ph["resid"] + 128.0
    noise = torch.from_numpy(rng.standard_normal(S) * 8.0).cuda()
    fs.set_photometric(I0 + noise, weight=1e-3, huber=10.0, band_sd=band_sd, presorted=True)

    def build_only():
        sv.build_associated(*frame_args, kw["rw"], kw["max_dist"], kw["huber"])

    def build_and_term():
        sv.build_associated(*frame_args, kw["rw"], kw["max_dist"], kw["huber"], colors=colors)

    def term_only():
        sv._add_photometric(fs.lw, sv._frame(depths, lws, fs.K, fs.Kinv, fs.scale, fs.center, fs.half, kw["max_dist"]), colors)

    def solve10():
        fs.gn_iteration(depths, lws, n_iters=10, **kw)

    def solve10_term():
        fs.gn_iteration(depths, lws, n_iters=10, colors=colors, **kw)

    say()
    say("1. dfh_gn_add_photometric beside the frame's fused build (us, median per round | round 2)")
    reset()
    build_and_term()
    torch.cuda.synchronize()
    r = rounds({"build": build_only, "build + term": build_and_term, "term alone": term_only}, args.reps, prep=None)
    say("  %d samples (%d scratch rows, %d active rows, %d valid data rows):" % (S, sv.n_rows, int(sv._ph["active"].sum()), int(sv.valid.sum())))
    for name, v in r.items():
        say("    %-14s %8.1f | %8.1f" % (name, v[0], v[1]))
    say()
    say("2. one frame's solve, 10 GN iterations in one library call (us, median per round | round 2)")
    reset()
    solve10_term()
    torch.cuda.synchronize()
    r = rounds({"without the term": solve10, "with the term": solve10_term, "without (b)": solve10, "with (b)": solve10_term}, args.reps, prep=reset)
    for name, v in r.items():
        say("    %-17s %9.1f | %9.1f" % (name, v[0], v[1]))
    if args.parent_lib:
        say()
        say("3. the one-call solve without the term: this build's library against the parent commit's (us, median per round | round 2)")
        plib = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _lib._SIGNATURES["dfh_gn_solve"]
        plib.dfh_gn_solve.restype, plib.dfh_gn_solve.argtypes = res, argt
        reset()
        solve10()
        frame = sv._frame(depths, lws, fs.K, fs.Kinv, fs.scale, fs.center, fs.half, kw["max_dist"])
        sp = sv._solve_params(kw["lm_abs"], kw["lm_rel"], 10, 0, 0.1, False)
        prob = sv._problem(fs.lw, kw["rw"], kw["huber"])

        def via(lib):
            def run():
                rc = lib.dfh_gn_solve(prob, frame, sp, current_stream_ptr())
                assert rc == 0, rc
            return run
        reset()
        via(sv.lib)()
        here = sv.node_dq.clone()
        reset()
        via(plib)()
        say("    node DQs after one solve identical between the two libraries: %s" % bool(torch.equal(here, sv.node_dq)))
        r = rounds({"this build": via(sv.lib), "parent": via(plib), "this build (b)": via(sv.lib), "parent (b)": via(plib)}, args.reps, prep=reset)
        for name, v in r.items():
            say("    %-15s %9.1f | %9.1f" % (name, v[0], v[1]))
        res, argt = _lib._SIGNATURES["dfh_gn_add_photometric"]
        plib.dfh_gn_add_photometric.restype, plib.dfh_gn_add_photometric.argtypes = res, argt
        say("   dfh_gn_add_photometric on the same structs through both libraries: bits, then the term alone (us)")
        reset()
        build_and_term()
        ph = sv._ph
        n_rows, ne, tile = sv.n_rows, int(sv.lib.dfh_gn_partial_doubles(k)), int(sv.lib.dfh_gn_tile_samples())
        n_tiles = (S + tile - 1) // tile                                    # the buffer: rows | {cost, 0} per tile | live flag per row

        def term_via(lib):
            fr = sv._frame(depths, lws, fs.K, fs.Kinv, fs.scale, fs.center, fs.half, kw["max_dist"])
            prob, term = sv._problem(fs.lw), sv._photo_term(colors, fr)

            def run():
                rc = lib.dfh_gn_add_photometric(prob, fr, term, current_stream_ptr())
                assert rc == 0, rc
            return run

        def outputs(lib):
            """build, then the term through `lib` into buffers of sentinels: what the term wrote and the system"""
            ph["partial"].fill_(-1.0)
            ph["active"].fill_(7)
            ph["view"].fill_(-7)
            ph["resid"].fill_(-7.0)
            build_only()
            term_via(lib)()
            torch.cuda.synchronize()
            p = ph["partial"]
            live = p[n_rows * ne + 2 * n_tiles:n_rows * ne + 2 * n_tiles + n_rows]
            rows = p[:n_rows * ne].view(n_rows, ne)[live == 1.0]          # (dead rows are never written: left out)
            return [t.clone() for t in (rows, p[n_rows * ne:n_rows * ne + 2 * n_tiles], live, sv.system, ph["active"], ph["view"], ph["resid"])]
        a, b = outputs(sv.lib), outputs(plib)
        names = ("live scratch rows", "tile-cost pairs", "live flags", "system after build + term", "active_out", "view_out", "resid_out")
        say("    %d of %d scratch rows live: %s" % (int(a[2].sum()), n_rows, ", ".join(
            "%s %s" % (n, "identical" if torch.equal(x, y) else "DIFFER") for n, x, y in zip(names, a, b))))
        r = rounds({"this build": term_via(sv.lib), "parent": term_via(plib), "this build (b)": term_via(sv.lib), "parent (b)": term_via(plib)},
                   args.reps)
        for name, v in r.items():
            say("      term alone, %-15s %8.1f | %8.1f" % (name, v[0], v[1]))
        new4, par4 = r["this build"] + r["this build (b)"], r["parent"] + r["parent (b)"]
        say("      term alone: this build's median of four %.1f, the parent's four span %.1f .. %.1f: %s"
            % (float(np.median(new4)), min(par4), max(par4), "no slower" if float(np.median(new4)) <= max(par4) else "SLOWER"))
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
