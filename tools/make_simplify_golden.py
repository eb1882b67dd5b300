"""Writes tests/golden/simplify_recovery.json from the numpy restatement of K24 (tests/simplify_np.py), on the CPU: the counts of
every case of tests/simplify_cases.py in both modes, the cube's corner and surface errors and the sphere's radial errors in both
modes.  The entry "hooks" (figures measured on the device by tests/test_gpu_simplify.py's write_canonical_mesh test, printed
there) is carried over from the file that exists.

    python tools/make_simplify_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simplify_np as SN                                     # noqa: E402
from simplify_cases import CASES, REG_CASES, cube_side, sphere   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "simplify_recovery.json")


def main():
    sv, sf = sphere()
    rec = SN.golden_record(CASES, REG_CASES, cube_side(), (sv, sf, 2.0, (12.3, 12.1, 11.7), 10.0))
    rec["about"] = ("K24 by tests/simplify_np.py. cube: six faces of 17 x 17 lattice vertices, spacing 1, offset 0.25, cell 3, origin the "
                    "minimum; sphere: r 10, 41 x 80 lattice, cell 2. Distances in the meshes' units.")
    if os.path.exists(OUT):
        old = json.load(open(OUT))
        if "hooks" in old:
            rec["hooks"] = old["hooks"]
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    q, m = rec["cube"]["quadric"], rec["cube"]["mean"]
    print("cube corner distance: quadric %.6f, mean %.6f (ratio %.4f)" % (q["corner_distance_max"], m["corner_distance_max"],
                                                                          q["corner_distance_max"] / m["corner_distance_max"]))
    print("cube mean surface error: quadric %.6f, mean %.6f" % (q["surface_error_mean"], m["surface_error_mean"]))
    for mode in ("quadric", "mean"):
        print("sphere %s: %s" % (mode, rec["sphere"][mode]))


if __name__ == "__main__":
    main()
