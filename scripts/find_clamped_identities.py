#!/usr/bin/env python3
"""Search for ambient-query identities whose disk point lies outside the unit circle, so that the clamp of
pz = sqrt(max(1 - (px^2 + py^2), 0)) acts (include/rtow.h, rtow_ambient_device): tests/ambient_cases.py CLAMPED_ID.

The disk point's radius is sqrt(w3 2^-32) and the sine polynomial overshoots by at most 1.3e-8 in px^2 + py^2, so only
identities with w3 >= 2^32 - 64 can qualify: about one in 2^26.  The search draws Philox request 0 of (pixel, sample) for
pixel < `pixels` and sample < 2^22 under `seed` (the vectorised tests/scatter_exact.philox_words, 2^16 identities at a
time), keeps those with such a w3 and evaluates px^2 + py^2 exactly for them (tests/ambient_exact.disk_exact).  Every
candidate is printed with px^2 + py^2 - 1; the ones above 0 are clamped.  No GPU and no library is needed.

   python scripts/find_clamped_identities.py [--seed 20261021] [--pixels 256] [--jobs 8]

With the defaults (2^30 identities, a few minutes on eight cores) it prints 13 candidates, of which one is clamped:
pixel 43, sample 1810345 (w3 = 2^32 - 2, px^2 + py^2 = 1 + 6.3e-9).
"""
import argparse
import sys
from multiprocessing import Pool
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "raytracing-one-weekend_amd"))

from scatter_exact import philox_words  # noqa: E402

LOG2_SAMPLES = 22
CHUNK = 1 << 16


def candidates(job):
    """The (pixel, sample, w3) with w3 >= 2^32 - 64 among one pixel's 2^22 samples."""
    seed, pixel = job
    pix = np.full(CHUNK, pixel, dtype=np.uint64)
    found = []
    for lo in range(0, 1 << LOG2_SAMPLES, CHUNK):
        sample = np.arange(lo, lo + CHUNK, dtype=np.uint64)
        w3 = np.asarray(philox_words(seed, pix, sample, 0)[3], dtype=np.uint64)
        for j in np.nonzero(w3 >= np.uint64((1 << 32) - 64))[0]:
            found.append((pixel, int(sample[j]), int(w3[j])))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--pixels", type=int, default=256)
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    import ambient_exact as ax

    with Pool(args.jobs) as pool:
        found = [c for part in pool.imap(candidates, [(args.seed, p) for p in range(args.pixels)]) for c in part]
    clamped = 0
    for pixel, sample, w3 in found:
        (px, py, pz), _, _ = ax.disk_exact(philox_words(args.seed, pixel, sample, 0))
        over = px * px + py * py - 1
        clamped += over.sign() > 0
        print(f"pixel {pixel} sample {sample}: w3 = 2^32 - {(1 << 32) - w3}, px^2 + py^2 - 1 = {float(over):.3e}"
              + ("  CLAMPED" if over.sign() > 0 else ""))
    print(f"{len(found)} candidates among {args.pixels} x 2^{LOG2_SAMPLES} identities under seed {args.seed}, "
          f"{clamped} clamped")


if __name__ == "__main__":
    main()
