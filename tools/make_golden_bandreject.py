#!/usr/bin/env python3
"""Generate tests/golden/g30_bandreject_draws.json by running the REFERENCE's band draw on the CPU.

Needs a checkout of the reference repository (the directory that holds its `cpc` package); run from the repository root:
    CPC_REFERENCE=DIR PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bandreject.py [--check]

The reference is imported unmodified under the stand-in modules of tools/make_golden_augment.py (importing that tool registers
them; nothing of it is run).  For every (seed, scaler) the file holds the 16 (low, high) pairs that 16 consecutive calls of
BandrejectAugment.generate_freq_mask(scaler) return after np.random.seed(seed) -- data only, as Python floats (json round-trips
them exactly).  `--check` regenerates and compares with the committed file instead of writing it."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_augment as stand_ins  # noqa: E402  (registers the stand-in modules and imports the reference)

OUT = os.path.join(stand_ins.ROOT, "tests", "golden", "g30_bandreject_draws.json")
SEEDS = (1234, 7, 2026)
SCALERS = (0.5, 1.0, 2.0)
DRAWS = 16


def record():
    draw = stand_ins.ref_aug.BandrejectAugment.generate_freq_mask
    cases = []
    for seed in SEEDS:
        for scaler in SCALERS:
            np.random.seed(seed)
            pairs = [[float(v) for v in draw(scaler)] for _ in range(DRAWS)]
            cases.append({"seed": seed, "scaler": scaler, "pairs": pairs})
    return {"draws": DRAWS, "cases": cases}


def main():
    got = record()
    if "--check" in sys.argv[1:]:
        with open(OUT) as fh:
            kept = json.load(fh)
        if kept != got:
            raise SystemExit(f"{OUT} differs from what the reference draws")
        print(OUT, "regenerates identically")
        return
    with open(OUT, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
