"""Writes tests/golden/smooth_recovery.json from the numpy restatement of K25 (tests/smooth_np.py), on the CPU: the rms radial
deviation and the mean radius of the noisy icosphere of tests/smooth_cases.py before and after ten Taubin iterations, and the
mean radius after twenty plain Laplacian passes.

    python tools/make_smooth_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import smooth_np as SN                                       # noqa: E402
from smooth_cases import CENTRE, RADIUS, noisy_icosphere     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "smooth_recovery.json")


def main():
    noisy, faces = noisy_icosphere()
    rec = SN.golden_record(noisy, faces, CENTRE, RADIUS)
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
