"""Writes the K13 fixtures tests/golden/k13_<scene>.npz: batch means of the independent float64 estimator of tests/converged_util.py.

    python tests/golden/make_converged.py [scene ...] [--batches B] [--spp S] [--seed N]

Budget condition: the film mean of a fixture has a relative standard error <= 0.1 % per channel; the script refuses to write a
fixture that misses it (raise --spp).  A file holds the B batch means (float64), the scene dict as JSON, the generator seed, the
batches, the samples per pixel of a batch, the wall time and the measured relative standard error per channel."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import converged_util as cu  # noqa: E402

# samples per pixel of one batch (B = 16 batches on 8 x 8 pixels) at which the budget condition was met
SPP = {"box": 16384, "box_direct": 8192, "box_tent": 12288, "meshlight_glass": 8192}
SEED = {"box": 1301, "box_direct": 1302, "box_tent": 1303, "meshlight_glass": 1304}
BUDGET = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=list(cu.SCENES))
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--seed", type=int, default=-1)
    a = ap.parse_args()
    for name in a.scenes:
        sc = cu.scene(name)
        spp = a.spp or SPP[name]
        seed = a.seed if a.seed >= 0 else SEED[name]
        t0 = time.time()
        films = cu.render_batches(sc, a.batches, spp, seed, progress=lambda b: print(f"  {name}: batch {b} at {time.time() - t0:.0f} s", flush=True))
        dt = time.time() - t0
        rel = cu.film_mean_rel_se(films)
        print(f"{name}: {a.batches} x {spp} spp = {a.batches * spp * films.shape[1] * films.shape[2] / 1e6:.1f} M paths, {dt:.0f} s, "
              f"film mean {films.mean(axis=(0, 1, 2))}, rel. standard error % {100 * rel}", flush=True)
        if not np.all(rel <= BUDGET):
            raise SystemExit(f"{name}: budget condition missed, raise --spp")
        np.savez_compressed(cu.fixture_path(name), batches=films, scene=json.dumps(sc), seed=seed, n_batches=a.batches, spp=spp,
                            seconds=dt, rel_se=rel)


if __name__ == "__main__":
    main()
