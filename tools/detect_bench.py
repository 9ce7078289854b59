"""Throughput of the GPU source detector (Context.scene_detect, csrc/detect.hip): fields per second for a batch of 259-px
fields, milliseconds for one 4096-px survey tile, and the numpy restatement's CPU time per 259-px field for comparison.
Fields: Gaussian noise plus ~40 Gaussian galaxies per 259 px (some blended).  GPU only; prints one JSON line.

    python tools/detect_bench.py [--batch 1024] [--tile 4096] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from debvader_amd import engine as E  # noqa: E402
from tests import detect_oracle as do  # noqa: E402


def _field(rng, H, W, n):
    f = 100.0 + rng.normal(0, 1.0, (H, W))
    ys, xs = rng.uniform(0, H, n), rng.uniform(0, W, n)
    sig, amp = rng.uniform(1.2, 4.0, n), rng.uniform(3.0, 60.0, n)
    for y, x, s, a in zip(ys, xs, sig, amp):
        r0, r1 = max(0, int(y - 5 * s)), min(H, int(y + 5 * s) + 1)
        c0, c1 = max(0, int(x - 5 * s)), min(W, int(x + 5 * s) + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        f[r0:r1, c0:c1] += a * np.exp(-0.5 * ((yy - y) ** 2 + (xx - x) ** 2) / s ** 2)
    return f


def _best(fn, repeat):
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--oracle-fields", type=int, default=4)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    F = 259
    base = np.stack([_field(rng, F, F, 40) for _ in range(16)])
    batch = np.ascontiguousarray(base[np.arange(a.batch) % 16])
    tile = _field(rng, a.tile, a.tile, int(40 * (a.tile / F) ** 2))[None]
    ctx = E.default_context()
    ctx.scene_detect(batch[:2])                                        # warm-up (module load, first allocations)
    tb, rb = _best(lambda: ctx.scene_detect(batch), a.repeat)
    tt, rt = _best(lambda: ctx.scene_detect(tile), a.repeat)
    t0 = time.perf_counter()
    for i in range(a.oracle_fields):
        do.detect(base[i])
    to = (time.perf_counter() - t0) / a.oracle_fields
    print(json.dumps({"batch": a.batch, "F": F, "batch_seconds": round(tb, 5), "fields_per_s": round(a.batch / tb, 1),
                      "objects_per_field": round(len(rb["x"]) / a.batch, 2), "tile": a.tile,
                      "tile_ms": round(1e3 * tt, 2), "tile_objects": int(len(rt["x"])),
                      "oracle_cpu_ms_per_field": round(1e3 * to, 2)}))


if __name__ == "__main__":
    main()
