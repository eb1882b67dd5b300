"""HIP-event timings of the landmark term (K16, csrc/dfh_landmarks.hip) on the bench's config-3 frame (256^3, 512 nodes, knn 4).

  1. dfh_gn_add_landmarks (rows kernel + accumulating gather) at L = 19 000 and 77 000 landmarks -- the vertex counts of the scene's
     256^3 and 512^3 meshes; the landmarks are that many band samples of the canonical volume, evenly strided -- beside the same
     frame's fused build (dfh_gn_build with the frame);
  2. one frame's solve (10 GN iterations, one library call) without landmarks and with 19 000 / 77 000;
  3. --parent-lib PATH: the one-call solve WITHOUT landmarks through this build's library and through the parent commit's
     (a second CDLL on the same problem structs), beside the spread of each variant timed twice; then dfh_gn_add_landmarks through
     both: the term's live scratch rows, tile-cost pairs and live flags, the system after build + term and active_out compared bit
     for bit, and the term alone timed through both (this build's median of its four medians against the parent's largest).

Variants alternate inside a round, medians of --reps (default 30) per round, every variant is timed in two rounds.

    python tools/kbench_landmarks.py [--reps 30] [--parent-lib build_variants/parent/libdfusion_hip.so] [--out profiles/r16_landmarks.txt]
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
    for a in (0.0, 40.0, -40.0):
        lw = scene.view_extrinsic(a)
        d = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
        kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    ident = torch.from_numpy(np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (N, 1))).cuda()
    fs = FrameSolver(K, scale, center, R / 2, knn=k, pcg_iters=10, distributed=False)
    fs.set_graph(node_pos, ident, node_w)
    S = fs.set_canonical(T, Wt, band=4.0)
    sv = fs.solver
    lw_cam = scene.view_extrinsic(0.0)
    off = np.array([0.6, -0.4, 0.3])
    depth = torch.from_numpy(scene.render_depth(K, lw_cam, H, W, dtype=np.float32, sphere_offset=off * scale,
                                                sphere_r=scene.SPHERE_R * 1.02)).cuda()
    kw = dict(rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.5)
    say("landmark term on the config-3 frame: %d^3, %d nodes, knn %d, %d samples; %d repetitions per round, two rounds" % (R, N, k, S, args.reps))

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

    def set_landmarks(L):
        if L == 0:
            sv.clear_landmarks()
            sv.landmark_weight = 0.0
            return
        sel = torch.linspace(0, S - 1, L, device="cuda").long()
        pts = sv.spos[sel].clone()
        tgt = pts + torch.tensor(off, dtype=torch.float64, device="cuda")
        fs.set_landmarks(pts, tgt, weight=1.0, huber=1.0, max_dist=3.0)

    def reset():
        sv.node_dq.copy_(ident)

    frame_args = (depth, fs.K, fs.Kinv, lw_cam, fs.scale, fs.center, fs.half, fs.lw)

    def build_only():
        w, sv.landmark_weight = sv.landmark_weight, 0.0
        sv.build_associated(*frame_args, kw["rw"], kw["max_dist"], kw["huber"])
        sv.landmark_weight = w

    def build_and_term():
        sv.build_associated(*frame_args, kw["rw"], kw["max_dist"], kw["huber"])

    def term_only():
        sv._add_landmarks(fs.lw)

    def solve10():
        fs.gn_iteration(depth, lw_cam, n_iters=10, **kw)

    say()
    say("1. dfh_gn_add_landmarks beside the frame's fused build (us, median per round | round 2)")
    for L in (19000, 77000):
        set_landmarks(L)
        reset()
        build_and_term()
        torch.cuda.synchronize()
        r = rounds({"build": build_only, "build + term": build_and_term, "term alone": term_only}, args.reps, prep=None)
        rows = sv._lm["plan"]["n_rows"]
        act = int(sv._lm["active"].sum())
        say("  L = %6d (%d scratch rows, %d active):" % (L, rows, act))
        for name, v in r.items():
            say("    %-14s %8.1f | %8.1f" % (name, v[0], v[1]))
    say()
    say("2. one frame's solve, 10 GN iterations in one library call (us, median per round | round 2)")
    res2 = {}
    for L in (0, 19000, 77000):
        set_landmarks(L)
        reset()
        solve10()
        torch.cuda.synchronize()
        res2[L] = rounds({"solve": solve10}, args.reps, prep=reset)["solve"]
    # (the three sizes cannot alternate repetition by repetition -- a landmark set is planned when it is set -- so the no-landmark
    # solve is timed again at the end: its two ends bracket the drift of the session)
    set_landmarks(0)
    reset()
    solve10()
    again = rounds({"solve": solve10}, args.reps, prep=reset)["solve"]
    for L in (0, 19000, 77000):
        say("    L = %6d: %9.1f | %9.1f" % (L, res2[L][0], res2[L][1]))
    say("    L =      0 again: %9.1f | %9.1f" % (again[0], again[1]))
    if args.parent_lib:
        say()
        say("3. the one-call solve without landmarks: this build's library against the parent commit's (us, median per round | round 2)")
        plib = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argt = _lib._SIGNATURES["dfh_gn_solve"]
        plib.dfh_gn_solve.restype, plib.dfh_gn_solve.argtypes = res, argt
        set_landmarks(0)
        reset()
        solve10()
        frame = sv._frame(depth, lw_cam, fs.K, fs.Kinv, fs.scale, fs.center, fs.half, kw["max_dist"])
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
        res, argt = _lib._SIGNATURES["dfh_gn_add_landmarks"]
        plib.dfh_gn_add_landmarks.restype, plib.dfh_gn_add_landmarks.argtypes = res, argt
        say("   dfh_gn_add_landmarks on the same structs through both libraries: bits, then the term alone (us)")
        for L in (19000, 77000):
            set_landmarks(L)
            reset()
            build_and_term()                                                # (plans the landmarks)
            plan = sv._lm["plan"]
            n_rows, ne = plan["n_rows"], int(sv.lib.dfh_gn_partial_doubles(k))
            tile = int(sv.lib.dfh_gn_tile_samples())
            n_tiles = (L + tile - 1) // tile                                # the buffer: rows | {cost, 0} per tile | live flag per row

            def term_via(lib):
                prob, term = sv._problem(fs.lw), sv._landmark_term()

                def run():
                    rc = lib.dfh_gn_add_landmarks(prob, term, current_stream_ptr())
                    assert rc == 0, rc
                return run

            def outputs(lib):
                """build, then the term through `lib` into a scratch buffer of sentinels: what the term wrote and the system"""
                plan["partial"].fill_(-1.0)
                sv._lm["active"].fill_(7)
                build_only()
                term_via(lib)()
                torch.cuda.synchronize()
                p = plan["partial"]
                live = p[n_rows * ne + 2 * n_tiles:]
                rows = p[:n_rows * ne].view(n_rows, ne)[live == 1.0]      # (dead rows are never written: left out)
                return [t.clone() for t in (rows, p[n_rows * ne:n_rows * ne + 2 * n_tiles], live, sv.system, sv._lm["active"])]
            a, b = outputs(sv.lib), outputs(plib)
            names = ("live scratch rows", "tile-cost pairs", "live flags", "system after build + term", "active_out")
            say("    L = %6d (%d of %d scratch rows live): %s" % (L, int(a[2].sum()), n_rows, ", ".join(
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
