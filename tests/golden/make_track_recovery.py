"""Writes tests/golden/track_recovery.json from the numpy restatement of K21 (tests/track_np.py) on the tracking scene
(tests/track_cases.py): the model is the scene rendered from the identity camera, the live frame the scene rendered from a camera
moved by motion(size), the prior the identity.  For every size the final rotation and translation error of
  "fine"   one level, the finest level's gate and cosine, all the schedule's iterations (19) at that level
  "loose"  one level, the coarsest level's gate and cosine, 19 iterations
  "pyramid" three levels with the per-level gates, cosines and iterations
Run from the repository root:  python tests/golden/make_track_recovery.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import track_cases as TC  # noqa: E402

SIZES = (0.5, 1.0, 1.5, 2.0)


def run(size):
    lw_true = TC.motion(size)
    live, _ = TC.render(lw_true)
    total = sum(TC.ITERS)
    out = {"applied_deg": 4.5 * size, "applied_m": 0.111 * size}
    for name, levels, gates, cosines, iters in (("fine", 1, TC.GATES[:1], TC.COSINES[:1], (total,)),
                                                ("loose", 1, TC.GATES[2:], TC.COSINES[2:], (total,)),
                                                ("pyramid", 3, TC.GATES, TC.COSINES, TC.ITERS)):
        T, stats = TC.track_np_pyramid(live, TC.IDENT, levels, gates, cosines, iters)
        deg, m = TC.pose_error(T, TC.IDENT, lw_true)
        out[name] = {"deg": deg, "m": m, "last_status": int(stats[0][-1, 29]), "count": int(stats[0][-1, 28])}
    return out


def main():
    rec = {"scene": "tests/track_cases.py", "gates": TC.GATES, "cosines": TC.COSINES, "iters": TC.ITERS, "max_jump": TC.MAX_JUMP, "lm_rel": TC.LM_REL,
           "sizes": {("%g" % s): run(s) for s in SIZES}}
    with open(os.path.join(HERE, "track_recovery.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for s, r in rec["sizes"].items():
        print(s, {k: (round(v["deg"], 4), round(v["m"] * 1e3, 3)) for k, v in r.items() if isinstance(v, dict)})


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
