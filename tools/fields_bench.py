"""Deblending many small fields: one engine call for all of them (DeblendFieldBatch) against a loop of single-field calls
(DeblendField), on one GPU.  M synthetic six-band fields of F px (Gaussian noise plus ~40 Gaussian galaxies per 259 px, some
blended, as tools/detect_bench.py makes them), detected once with detect_objects_batch; then, alternating, after a warm-up,

    loop :  for every field  DeblendField(net, field).deblend_field(d, on_device=True)
    batch:  DeblendFieldBatch(net, fields).deblend_fields(d, on_device=True)

for both engine dtypes, --repeat times each; stamps/s and fields/s per repetition, the median and the spread (max - min
over the median).  Also, on --default-fields fields, the default (stamps returned) mode of both and optimise_positions().
GPU only; prints a table and one JSON line.

    python tools/fields_bench.py [--fields 1024] [--size 259] [--repeat 5] [--max-batch 8192]

--epistemic N runs another comparison INSTEAD: the predicted mean / stddev / epistemic fields and the
cuts of every field with N Monte-Carlo samples per galaxy,

    before:  for every field, the engine calls DeblendField(epistemic_uncertainty_estimation=True) made before the estimate
             became a pipeline stage: deblend_field() (infer_cutouts_keep), deblend_epistemic() on the stamps (infer_mc:
             float32 stamps up again, a second encoder pass, std stamps down), get_predicted_field() (three composites of
             stamps sent up once more).  An emulation, not the old code: the same engine calls with the
             same arguments, three composites per field (mean and stddev in get_predicted_field(), the std stamps in a
             call of their own) and the cut on the host, as before; it stacks the cutouts into one array once more than
             the old path did (a host copy of 167 KB per stamp)
    loop  :  for every field  DeblendField(..., epistemic_uncertainty_estimation=True): deblend_field() +
             get_predicted_field() as they are now (N = 100 only: the class fixes the reference's 100 samples)
    batch :  DeblendFieldBatch(net, fields).deblend_fields(d, on_device=True, epistemic_uncertainty_estimation=True,
             epistemic_samples=N) + get_predicted_fields()

alternating, --repeat times each, both engines.

--optimise-positions runs a third comparison INSTEAD: fields with every galaxy at its fitted sub-pixel
position (distances rounded to integers, as the device path needs),

    host  :  db.deblend_fields(d); db.optimise_positions(); db.get_predicted_fields(); db.get_residual_fields()
             (stamps to the host, their r band up again for the fit, all of them up again for three composites per field)
    device:  db.deblend_fields(d, on_device=True, optimise_positions=True); get_predicted_fields(); get_residual_fields()

alternating, --repeat times each, both engines; --profile-one: warm up, one fp32 device call, exit (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from debvader_amd.deblend.field_deblender import DeblendField, DeblendFieldBatch  # noqa: E402
from debvader_amd.detect.detection import detect_objects_batch  # noqa: E402
from debvader_amd.model import model  # noqa: E402

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])


def _field(rng, F, n, nb=6):
    f = np.zeros((F, F))
    ys, xs = rng.uniform(0, F, n), rng.uniform(0, F, n)
    sig, amp = rng.uniform(1.2, 4.0, n), rng.uniform(3.0, 60.0, n)
    for y, x, s, a in zip(ys, xs, sig, amp):
        r0, r1 = max(0, int(y - 5 * s)), min(F, int(y + 5 * s) + 1)
        c0, c1 = max(0, int(x - 5 * s)), min(F, int(x + 5 * s) + 1)
        yy, xx = np.mgrid[r0:r1, c0:c1]
        f[r0:r1, c0:c1] += a * np.exp(-0.5 * ((yy - y) ** 2 + (xx - x) ** 2) / s ** 2)
    return f[:, :, None] * rng.uniform(0.4, 1.0, nb) + rng.normal(0, 1.0, (F, F, nb))


def _loop(net, fields, dists, on_device):
    n = 0
    for m in range(len(fields)):
        r = DeblendField(net, fields[m:m + 1]).deblend_field(dists[m], on_device=on_device)
        n += 0 if isinstance(r, dict) else len(r)
    return n


def _batch(net, fields, dists, on_device):
    return sum(len(r) for r in DeblendFieldBatch(net, fields).deblend_fields(dists, on_device=on_device))


def _before_field(net, field, d, nsamples):
    from debvader_amd.deblend_cutout.deblender import deblend_epistemic

    db = DeblendField(net, field)
    r = db.deblend_field(d)
    if isinstance(r, dict):
        return 0
    rows = np.array(list(r["cutout_images"]))
    _, eps = deblend_epistemic(net, rows, n_samples=nsamples)
    eps = eps.astype(np.float64)
    norm = np.array([np.sum(e[:, :, 2]) for e in eps]) / np.array([np.sum(m[:, :, 2]) for m in r["output_images_mean"]])
    r["passed_cuts"] = r["passed_cuts"] & ~(norm > 100.0)
    db.get_predicted_field()
    db._ctx.scene_composite(np.zeros(field.shape[1:]), eps, DeblendField._positions(r))
    return len(r)


def _epistemic_loop(net, fields, dists):
    n = 0
    for m in range(len(fields)):
        db = DeblendField(net, fields[m:m + 1], epistemic_uncertainty_estimation=True)
        r = db.deblend_field(dists[m])
        if not isinstance(r, dict):
            db.get_predicted_field()
            n += len(r)
    return n


def _epistemic_batch(net, fields, dists, nsamples):
    db = DeblendFieldBatch(net, fields)
    res = db.deblend_fields(dists, on_device=True, epistemic_uncertainty_estimation=True, epistemic_samples=nsamples)
    db.get_predicted_fields()
    return sum(len(r) for r in res)


def _epistemic_leg(a, fields, quiet, redirect_stdout):
    M, F, ns = len(fields), fields.shape[1], a.epistemic
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "epistemic_samples": ns}
    dists = None
    for dtype in ("float32", "bf16"):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; {ns} Monte-Carlo samples; "
                  f"max_batch {a.max_batch}")
        legs = {"before": lambda: sum(_before_field(net, fields[m:m + 1], dists[m], ns) for m in range(M)),
                "batch": lambda: _epistemic_batch(net, fields, dists, ns)}
        if ns == 100:
            legs["loop"] = lambda: _epistemic_loop(net, fields, dists)
        times = {k: [] for k in legs}
        n = 0
        with redirect_stdout(quiet):
            _before_field(net, fields[:1], dists[0], ns)                               # warm-up
            _epistemic_batch(net, fields[:min(M, 64)], dists[:min(M, 64)], ns)
            if a.profile_one:                  # one batched call, for a kernel trace
                _epistemic_batch(net, fields, dists, ns)
                net._core.engine.close()
                return
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} epistemic {k}", t, n, M))
            result[dtype][k + "_ms"] = [round(1e3 * x, 2) for x in t]
        tb, tl = np.array(times["batch"]), np.array(times["before"])
        print(f"{dtype} epistemic before / batch: {float(np.median(tl) / np.median(tb)):.2f} x  (slowest batch "
              f"{1e3 * tb.max():.1f} ms, fastest before {1e3 * tl.min():.1f} ms)")
        result[dtype]["factor"] = round(float(np.median(tl) / np.median(tb)), 3)
        net._core.engine.close()
    print(json.dumps(result))


def _fit_host(net, fields, dists):
    db = DeblendFieldBatch(net, fields)
    res = db.deblend_fields(dists)
    db.optimise_positions()
    db.get_predicted_fields()
    db.get_residual_fields()
    return sum(len(r) for r in res)


def _fit_device(net, fields, dists):
    db = DeblendFieldBatch(net, fields)
    res = db.deblend_fields(dists, on_device=True, optimise_positions=True)
    db.get_predicted_fields()
    db.get_residual_fields()
    return sum(len(r) for r in res)


def _fit_leg(a, fields, quiet, redirect_stdout):
    M, F = len(fields), fields.shape[1]
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "optimise_positions": True}
    dists = None
    for dtype in ("float32", "bf16"):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; max_batch {a.max_batch}")
        with redirect_stdout(quiet):
            _fit_host(net, fields[:8], dists[:8])                                      # warm-up
            _fit_device(net, fields, dists)
            if a.profile_one:
                _fit_device(net, fields, dists)
                net._core.engine.close()
                return
            th, td, n = _alternate(lambda: _fit_host(net, fields, dists), lambda: _fit_device(net, fields, dists), a.repeat)
        print(_row(f"{dtype} fitted fields, host", th, n, M))
        print(_row(f"{dtype} fitted fields, device", td, n, M))
        factor = float(np.median(th) / np.median(td))
        print(f"{dtype} fitted fields host / device: {factor:.2f} x  (slowest device {1e3 * td.max():.1f} ms, fastest host "
              f"{1e3 * th.min():.1f} ms)")
        result[dtype] = {"stamps": n, "host_ms": [round(1e3 * x, 2) for x in th], "device_ms": [round(1e3 * x, 2) for x in td],
                         "factor": round(factor, 3)}
        net._core.engine.close()
    print(json.dumps(result))


def _alternate(fa, fb, repeat):
    ta, tb, n = [], [], 0
    for _ in range(repeat):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            n = fn()
            ts.append(time.perf_counter() - t0)
    return np.array(ta), np.array(tb), n


def _row(label, t, stamps, fields):
    med = float(np.median(t))
    return (f"{label:<34s} {stamps / med:12.0f} stamps/s {fields / med:10.1f} fields/s   median {1e3 * med:9.1f} ms   "
            f"spread {100 * (t.max() - t.min()) / med:5.1f} %   runs " + " ".join(f"{1e3 * x:.1f}" for x in t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=1024)
    ap.add_argument("--size", type=int, default=259)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=8192)
    ap.add_argument("--default-fields", type=int, default=64)
    ap.add_argument("--epistemic", type=int, default=0, help="Monte-Carlo samples: run the epistemic comparison instead")
    ap.add_argument("--optimise-positions", action="store_true", help="run the fitted-positions comparison instead")
    ap.add_argument("--profile-one", action="store_true",
                    help="with --epistemic or --optimise-positions: warm up, one fp32 batched call, exit")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    import io
    from contextlib import redirect_stdout
    quiet = io.StringIO()                      # the classes print the reference's notes about dropped galaxies
    if a.epistemic > 0:
        _epistemic_leg(a, fields, quiet, redirect_stdout)
        return
    if a.optimise_positions:
        _fit_leg(a, fields, quiet, redirect_stdout)
        return
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat}
    dists = None
    for dtype in ("float32", "bf16"):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.asarray(d, dtype=np.float64).reshape(-1, 2) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections "
                  f"({sum(len(d) for d in dists) / M:.1f} per field); max_batch {a.max_batch}")
        with redirect_stdout(quiet):
            _loop(net, fields[:8], dists[:8], True)                                   # warm-up
            _batch(net, fields, dists, True)
            tl, tb, n = _alternate(lambda: _loop(net, fields, dists, True), lambda: _batch(net, fields, dists, True), a.repeat)
        print(_row(f"{dtype} on_device loop", tl, n, M))
        print(_row(f"{dtype} on_device batch", tb, n, M))
        factor = float(np.median(tl) / np.median(tb))
        print(f"{dtype} on_device batch / loop: {factor:.2f} x  (slowest batch {1e3 * tb.max():.1f} ms, fastest loop "
              f"{1e3 * tl.min():.1f} ms)")
        result[dtype] = {"stamps": n, "loop_ms": [round(1e3 * x, 2) for x in tl], "batch_ms": [round(1e3 * x, 2) for x in tb],
                         "factor": round(factor, 3), "batch_stamps_per_s": round(n / float(np.median(tb)), 1),
                         "loop_stamps_per_s": round(n / float(np.median(tl)), 1)}
        # default mode (stamps returned) and the position fit, on fewer fields: 334 KB of results per stamp on the host
        Md = min(M, a.default_fields)
        with redirect_stdout(quiet):
            _batch(net, fields[:Md], dists[:Md], False)
            tl, tb, n = _alternate(lambda: _loop(net, fields[:Md], dists[:Md], False),
                                   lambda: _batch(net, fields[:Md], dists[:Md], False), a.repeat)
        print(_row(f"{dtype} default loop ({Md} fields)", tl, n, Md))
        print(_row(f"{dtype} default batch ({Md} fields)", tb, n, Md))
        result[dtype]["default"] = {"fields": Md, "stamps": n, "loop_ms": [round(1e3 * x, 2) for x in tl],
                                    "batch_ms": [round(1e3 * x, 2) for x in tb]}
        if dtype == "float32":
            with redirect_stdout(quiet):
                db = DeblendFieldBatch(net, fields[:Md])
                db.deblend_fields(dists[:Md])
                singles = [DeblendField(net, fields[m:m + 1]) for m in range(Md)]

                def fit_loop():
                    for m in range(Md):
                        if len(db.res_deblend[m]):
                            singles[m].optimise_positions(db.res_deblend[m])
                    return n

                def fit_batch():
                    db.optimise_positions()
                    return n

                fit_batch()
                tl, tb, _ = _alternate(fit_loop, fit_batch, a.repeat)
            print(_row(f"optimise_positions loop ({Md} fields)", tl, n, Md))
            print(_row(f"optimise_positions batch ({Md} fields)", tb, n, Md))
            result["optimise_positions"] = {"fields": Md, "galaxies": n, "loop_ms": [round(1e3 * x, 2) for x in tl],
                                            "batch_ms": [round(1e3 * x, 2) for x in tb]}
        net._core.engine.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
