"""Throughput of the batched position fit (dv_scene_fit_shifts): galaxies/s for N galaxies on a 259-px field with 59-px
stamps, and the mean Newton iterations.  Nine Gaussian galaxies sit 0.5-2 px from integer grid distances in a noisy field;
each fit takes one of them with a perturbed stamp, so every galaxy has an interior optimum to find.  GPU only; prints one JSON line.

    python tools/posfit_bench.py [--n 8192] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from debvader_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fractional", type=float, default=0.0, help="share of galaxies with a fractional distance")
    a = ap.parse_args()
    F, cs, n = 259, 59, a.n
    po = (F - cs) // 2
    rng = np.random.default_rng(0)
    y, x = np.mgrid[:cs, :cs] - (cs - 1) / 2.0
    # nine galaxies on a 3 x 3 grid, 84 px apart, drawn into a noisy field 0.5-2 px from integer distances
    grid = np.array([[a, b] for a in (-84, 0, 84) for b in (-84, 0, 84)], np.float64)
    sig = rng.uniform(2.0, 5.0, size=9)
    amp = rng.uniform(0.5, 5.0, size=9)
    true = grid + rng.uniform(0.5, 2.0, size=(9, 2)) * rng.choice([-1.0, 1.0], size=(9, 2))
    field = rng.normal(0, 0.05, size=(F, F))
    for k in range(9):
        g = amp[k] * np.exp(-0.5 * (x ** 2 + y ** 2) / sig[k] ** 2)
        pad = np.zeros((F, F))
        pad[po:po + cs, po:po + cs] = g
        field += scipy.ndimage.shift(pad, true[k])
    # n fits: galaxy i % 9 with a perturbed model stamp (as a network output would be), at its grid distance
    gal = np.arange(n) % 9
    sig_i = sig[gal] * rng.uniform(0.9, 1.1, size=n)
    amp_i = amp[gal] * rng.uniform(0.9, 1.1, size=n)
    stamps = amp_i[:, None, None] * np.exp(-0.5 * (x[None] ** 2 + y[None] ** 2) / sig_i[:, None, None] ** 2)
    dist = grid[gal].copy()
    k = int(n * a.fractional)
    dist[:k] += rng.uniform(-0.5, 0.5, size=(k, 2))
    ctx = E.default_context()
    ctx.scene_fit_shifts(field, stamps[:4], dist[:4])                 # warm-up (module load, first allocations)
    times, r = [], None
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        r = ctx.scene_fit_shifts(field, stamps, dist)
        times.append(time.perf_counter() - t0)
    t = min(times)
    st = r["status"]
    print(json.dumps({"n": n, "F": F, "cs": cs, "fractional": a.fractional, "seconds": round(t, 5),
                      "galaxies_per_s": round(n / t, 1), "mean_iters": round(float(r["iters"].mean()), 3),
                      "max_iters": int(r["iters"].max()), "converged": int((st == 0).sum()), "on_bound": int((st == 1).sum()),
                      "iter_limit": int((st == 2).sum()), "stalled": int((st == 3).sum())}))


if __name__ == "__main__":
    main()
