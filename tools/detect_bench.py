"""Throughput of the GPU source detector (Context.scene_detect, csrc/detect.hip): fields per second for a batch of 259-px
fields, milliseconds for one 4096-px survey tile, and the numpy restatement's CPU time per 259-px field for comparison.
Fields: Gaussian noise plus ~40 Gaussian galaxies per 259 px (some blended).  GPU only; prints one JSON line.

    python tools/detect_bench.py [--batch 1024] [--tile 4096] [--repeat 3]

--weights [--filter matched]: the same two workloads with a per-pixel noise map and a mask (inverse
variances, every 97th column and one block per 259 px masked), the unweighted and the weighted leg alternating in one
process, --runs (5) timed runs each; prints the medians, the spread (min .. max) and the ratio of the medians.

    python tools/detect_bench.py --weights [--filter matched] [--runs 5]

--bands 0,1,2,3,4,5: the same two workloads with those bands combined (Context.scene_detect_multiband on
interleaved six-band fields whose band 2 is the single-band leg's field), the single-band and the multi-band leg alternating
in one process as above.

    python tools/detect_bench.py --bands 0,1,2,3,4,5 [--filter matched] [--runs 5]

--objects: the same two workloads through Context.scene_detect_objects: the existing call, the new call
with the object columns, and the new call with the columns and the segmentation map, the three legs alternating in one process.

    python tools/detect_bench.py --objects [--runs 5]

--clean: the same two workloads through Context.scene_detect_objects and through Context.scene_detect_clean (DESIGN.md section
7zc: the cleaning pass behind the same detection), both with the columns and the segmentation map, alternating in one process;
also how many objects the pass merged away.

    python tools/detect_bench.py --clean [--clean-param 1.0] [--runs 5]
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


def _weights(shape):
    """inverse variances of the fields' unit noise, with every 97th column and a 9 x 13 block per 259 px masked"""
    w = np.ones(shape)
    w[..., :, 50::97] = 0.0
    for r in range(100, shape[-2], 259):
        for c in range(120, shape[-1], 259):
            w[..., r:r + 9, c:c + 13] = 0.0
    return w


def _alternate(plain, weighted, runs):
    """runs timed calls of each leg, alternating: per leg (median, min, max) seconds and the last result"""
    tp, tw, rp, rw = [], [], None, None
    for _ in range(runs):
        t0 = time.perf_counter()
        rp = plain()
        t1 = time.perf_counter()
        rw = weighted()
        t2 = time.perf_counter()
        tp.append(t1 - t0)
        tw.append(t2 - t1)
    stats = lambda t: (float(np.median(t)), min(t), max(t))
    return stats(tp), stats(tw), rp, rw


def main_weighted(a, ctx, batch, tile):
    # thresh in units of the pixel's sigma: 1.5 on the smoothed map of "conv" as in the unweighted leg, 5 on the matched
    # filter's S, which is in units of the FILTERED noise (1.5 there is a forest of noise peaks)
    kw = dict(noise="absolute", filter_type=a.filter, thresh=5.0 if a.filter == "matched" else 1.5)
    wb, wt = _weights(batch.shape), _weights(tile.shape)
    ctx.scene_detect(batch[:2], weights=wb[:2], **kw)                  # warm-up of the weighted kernels
    out = {"batch": a.batch, "F": batch.shape[1], "tile": a.tile, "filter": a.filter, "noise": "absolute", "thresh": kw["thresh"],
           "runs": a.runs,
           "masked_fraction": round(float((wb[0] == 0).mean()), 4)}
    for name, f, w, scale in (("batch", batch, wb, 1.0), ("tile", tile, wt, 1e3)):
        p, q, rp, rw = _alternate(lambda: ctx.scene_detect(f), lambda: ctx.scene_detect(f, weights=w, **kw), a.runs)
        unit = "seconds" if name == "batch" else "ms"
        for leg, t, r in (("unweighted", p, rp), ("weighted", q, rw)):
            out[f"{name}_{leg}_{unit}_median"] = round(scale * t[0], 5)
            out[f"{name}_{leg}_{unit}_min_max"] = [round(scale * t[1], 5), round(scale * t[2], 5)]
            out[f"{name}_{leg}_objects"] = int(len(r["x"]))
        out[f"{name}_weighted_over_unweighted"] = round(q[0] / p[0], 4)
    print(json.dumps(out))


def _six_bands(rng, f):
    """(.., H, W) -> (.., H, W, 6): band 2 is f, the others f's sources at another amplitude on a sky and noise of their own"""
    out = np.empty(f.shape + (6,))
    for b, (amp, sky, sig) in enumerate(((0.6, 50.0, 1.0), (0.8, 20.0, 1.5), (1.0, 100.0, 1.0), (1.1, 10.0, 1.25), (1.2, 5.0, 0.8),
                                         (0.9, 200.0, 2.0))):
        out[..., b] = f if b == 2 else sky + amp * (f - 100.0) + rng.normal(0, sig, f.shape[-2:])
    return out


def main_bands(a, ctx, batch, tile):
    bands = [int(b) for b in a.bands.split(",")]
    rng = np.random.default_rng(1)
    # the combined threshold is in units of the combined pixel's sigma: 1.5 on the smoothed map as in the single-band leg, 5 on
    # the matched filter's S
    kw = dict(bands=bands, filter_type=a.filter, thresh=5.0 if a.filter == "matched" else 1.5)
    mb, mt = _six_bands(rng, batch), _six_bands(rng, tile)
    ctx.scene_detect_multiband(mb[:2], **kw)                           # warm-up of the multi-band kernels
    out = {"batch": a.batch, "F": batch.shape[1], "tile": a.tile, "bands": bands, "filter": a.filter, "thresh": kw["thresh"],
           "runs": a.runs}
    for name, f, m, scale in (("batch", batch, mb, 1.0), ("tile", tile, mt, 1e3)):
        p, q, rp, rq = _alternate(lambda: ctx.scene_detect(f), lambda: ctx.scene_detect_multiband(m, **kw), a.runs)
        unit = "seconds" if name == "batch" else "ms"
        for leg, t, r in (("single", p, rp), ("multiband", q, rq)):
            out[f"{name}_{leg}_{unit}_median"] = round(scale * t[0], 5)
            out[f"{name}_{leg}_{unit}_min_max"] = [round(scale * t[1], 5), round(scale * t[2], 5)]
            out[f"{name}_{leg}_objects"] = int(len(r["x"]))
        out[f"{name}_multiband_over_single"] = round(q[0] / p[0], 4)
    print(json.dumps(out))


def main_objects(a, ctx, batch, tile):
    ctx.scene_detect_objects(batch[:2], segmentation_map=True)         # warm-up of the objects kernel
    legs = (("existing", lambda f: ctx.scene_detect(f)), ("columns", lambda f: ctx.scene_detect_objects(f)),
            ("columns_segmap", lambda f: ctx.scene_detect_objects(f, segmentation_map=True)))
    out = {"batch": a.batch, "F": batch.shape[1], "tile": a.tile, "runs": a.runs}
    for name, f, scale in (("batch", batch, 1.0), ("tile", tile, 1e3)):
        times = {leg: [] for leg, _ in legs}
        res = {}
        for _ in range(a.runs):                                        # the three legs alternating
            for leg, fn in legs:
                t0 = time.perf_counter()
                res[leg] = fn(f)
                times[leg].append(time.perf_counter() - t0)
        unit = "seconds" if name == "batch" else "ms"
        for leg, _ in legs:
            t = times[leg]
            out[f"{name}_{leg}_{unit}_median"] = round(scale * float(np.median(t)), 5)
            out[f"{name}_{leg}_{unit}_min_max"] = [round(scale * min(t), 5), round(scale * max(t), 5)]
            out[f"{name}_{leg}_objects"] = int(len(res[leg]["x"]))
        for leg in ("columns", "columns_segmap"):
            out[f"{name}_{leg}_over_existing"] = round(float(np.median(times[leg]) / np.median(times["existing"])), 4)
    print(json.dumps(out))


def main_clean(a, ctx, batch, tile):
    ctx.scene_detect_clean(batch[:2], segmentation_map=True, clean_param=a.clean_param)      # warm-up of the clean kernels
    legs = (("objects", lambda f: ctx.scene_detect_objects(f, segmentation_map=True)),
            ("clean", lambda f: ctx.scene_detect_clean(f, segmentation_map=True, clean_param=a.clean_param)))
    out = {"batch": a.batch, "F": batch.shape[1], "tile": a.tile, "runs": a.runs, "clean_param": a.clean_param}
    for name, f, scale in (("batch", batch, 1.0), ("tile", tile, 1e3)):
        times = {leg: [] for leg, _ in legs}
        res = {}
        for _ in range(a.runs):                                        # the two legs alternating
            for leg, fn in legs:
                t0 = time.perf_counter()
                res[leg] = fn(f)
                times[leg].append(time.perf_counter() - t0)
        unit = "seconds" if name == "batch" else "ms"
        for leg, _ in legs:
            t = times[leg]
            out[f"{name}_{leg}_{unit}_median"] = round(scale * float(np.median(t)), 5)
            out[f"{name}_{leg}_{unit}_min_max"] = [round(scale * min(t), 5), round(scale * max(t), 5)]
            out[f"{name}_{leg}_objects"] = int(len(res[leg]["x"]))
        assert int(res["clean"]["n_raw"].sum()) == len(res["objects"]["x"])
        out[f"{name}_merged_away"] = int(len(res["objects"]["x"]) - len(res["clean"]["x"]))
        out[f"{name}_largest_nmerged"] = int(res["clean"]["nmerged"].max(initial=0))
        out[f"{name}_clean_over_objects"] = round(float(np.median(times["clean"]) / np.median(times["objects"])), 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--oracle-fields", type=int, default=4)
    ap.add_argument("--weights", action="store_true", help="alternate the unweighted and the weighted detector")
    ap.add_argument("--filter", choices=("conv", "matched"), default="conv")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bands", default=None, help="comma-separated band numbers: alternate the single-band and the multi-band "
                                                  "detector")
    ap.add_argument("--objects", action="store_true", help="alternate the existing call and Context.scene_detect_objects "
                                                           "without and with the segmentation map")
    ap.add_argument("--clean", action="store_true", help="alternate Context.scene_detect_objects and "
                                                         "Context.scene_detect_clean, both with the segmentation map")
    ap.add_argument("--clean-param", type=float, default=1.0)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    F = 259
    base = np.stack([_field(rng, F, F, 40) for _ in range(16)])
    batch = np.ascontiguousarray(base[np.arange(a.batch) % 16])
    tile = _field(rng, a.tile, a.tile, int(40 * (a.tile / F) ** 2))[None]
    ctx = E.default_context()
    ctx.scene_detect(batch[:2])                                        # warm-up (module load, first allocations)
    if a.weights:
        return main_weighted(a, ctx, batch, tile)
    if a.bands:
        return main_bands(a, ctx, batch, tile)
    if a.objects:
        return main_objects(a, ctx, batch, tile)
    if a.clean:
        return main_clean(a, ctx, batch, tile)
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
