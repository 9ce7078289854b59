"""Iterative deblending of many small fields: the fields resident on the GPU (IterativeDeblendFieldBatch, DESIGN.md section
7h) against a Python loop of IterativeDeblendField over the same fields - the form that existed before - on one GPU.
M synthetic six-band fields of F px as tools/fields_bench.py makes them; then, alternating, after a warm-up,

    loop :  for every field  IterativeDeblendField(net, field).iterative_deblending()
    batch:  IterativeDeblendFieldBatch(net, fields).iterative_deblending(mode="reference")

for both engine dtypes (--dtype picks one), --repeat times each: fields/s per repetition, the median and the spread (max -
min over the median).  Both forms apply the reference's residual and stopping rule, so they make the same passes on a field
until the single-field class meets an empty pass (which it records once more, section 7h).  The bytes that cross the host
link per pass are counted from the passes the run made: field-sized arrays and float32 stamps in the loop, catalogues
and per-stamp scalars in the batched form.  GPU only; prints a table and one JSON line.

    python tools/iterative_bench.py [--fields 64] [--size 259] [--repeat 5] [--max-batch 8192] [--dtype both]
                                    [--measure] [--no-fields] [--fit-flux [--fit-weights] [--fit-sky 0|1] [--fit-nonneg]
                                                                          [--fit-groups]] [--crowded ROWS_PER_PASS]

--profile-one: warm up, run the batched form once (float32 unless --dtype says otherwise) and exit - for a kernel trace; with
--measure --fit-flux that one run is the catalogue with the joint flux fit (with --fit-groups: the grouped one).
--measure / --no-fields: instead of the loop, the batched form against itself through
iterative_catalogue with measure=True, blendedness=True and / or return_fields=False - every combination the switches name,
alternating from the same seed counter: the cost of the catalogue stage and of the three field-sized downloads.
--fit-flux (with --measure): one more form per catalogue form, the same call with fit_flux=True - the
joint flux fit of all passes after the last one - and the milliseconds per loop and microseconds per galaxy it adds.
--fit-weights (uniform random inverse variances with a tenth of the pixels masked), --fit-sky and --fit-nonneg pick the variant.
--fit-groups (with --fit-flux, without --fit-sky and --fit-nonneg): one more form beside every form with
the fit, the same call with fit_groups=True - the joint fit by blend groups, in place on the kept stamps - and what it costs or
saves beside the dense fit.
--crowded ROWS_PER_PASS (a leg of its own, after the others): ONE field of --size px whose stamps fall in clusters - starts
inside 20-pixel boxes on a pitch that keeps the clusters apart -, two measured passes of ROWS_PER_PASS windows each on a
FieldSet with the stamps kept, then FieldSet.fit_flux_groups --repeat times: the median of the call, the groups, and whether the
dense FieldSet.fit_flux takes the field at all.
"""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fields_bench import ARCH, _field  # noqa: E402
from debvader_amd.deblend_iterative import IterativeDeblendField, IterativeDeblendFieldBatch  # noqa: E402
from debvader_amd.model import model  # noqa: E402

CS, NB = 59, 6


def _loop(net, fields):
    """-> galaxies deblended, [(detections, galaxies) per deblending pass and field]"""
    n, passes = 0, []
    for m in range(len(fields)):
        it = IterativeDeblendField(net, fields[m:m + 1])
        it.iterative_deblending()
        n += sum(it.nb_of_deblended_galaxies)
        passes += list(zip(it.nb_of_detected_objects, it.nb_of_deblended_galaxies))
        passes += [(0, 0)] * (len(it.mse) - len(it.nb_of_deblended_galaxies))       # passes that found nothing to deblend
    return n, passes


def _batch(net, fields, **kw):
    """-> galaxies deblended, [(active fields, detections, galaxies) per pass]"""
    it = IterativeDeblendFieldBatch(net, fields)
    res = it.iterative_catalogue(mode="reference", **kw) if kw else it.iterative_deblending(mode="reference")
    passes = [(sum(1 for c in g if c > 0), sum(d), sum(g)) for d, g in zip(it.nb_of_detected_objects,
                                                                         it.nb_of_deblended_galaxies)]
    return sum(len(r) for r in res), passes


def loop_pass_bytes(F, detections, galaxies):
    """Host-link bytes of one pass of IterativeDeblendField on one field: the r band to the detector and its catalogue
    back; the float64 residual and the windows to dv_infer_cutouts_keep, float32 mean and stddev stamps back; the field and
    the float64 mean stamps to dv_scene_composite, the residual back."""
    field = F * F * NB * 8
    up = F * F * 8 + (field + galaxies * 8 if galaxies else 0) + field + galaxies * (CS * CS * NB * 8 + 16)
    down = detections * 44 + galaxies * 2 * CS * CS * NB * 4 + field
    return up + down


def batch_pass_bytes(M, detections, galaxies):
    """Host-link bytes of one pass of IterativeDeblendFieldBatch over M fields: the active mask up, the catalogue (44 bytes
    per detection, offsets and globalrms per field) down; windows, placements and field numbers up (20 bytes per galaxy
    plus the field table), mse_center and one field_mse per field down."""
    return M + detections * 44 + (M + 1) * 8 + M * 8 + galaxies * 20 + (M + 1) * 4 + galaxies * 8 + M * 8


def _crowded(eng, F, per_pass, repeat, dtype):
    """One field whose stamps fall in clusters that cannot touch, two measured passes with the stamps kept, the grouped joint
    fit timed on its own"""
    from debvader_amd._lib import DvError

    box = 20
    pitch = CS + box + 13
    side = max(1, (F - CS - box) // pitch + 1)
    rng = np.random.default_rng(2)
    field = _field(rng, F, int(round(40 * (F / 259) ** 2)))[None]
    fs = eng.open_field_set(field)
    fs.keep_stamps()
    try:
        for p in range(2):
            k = np.arange(per_pass) % (side * side)
            starts = (np.stack([pitch * (k // side), pitch * (k % side)], axis=1) + rng.integers(0, box, size=(per_pass, 2))).astype(np.int32)
            fs.deblend_pass_measure(starts, starts, np.array([0, per_pass], np.int64), seed=7 + p)
        try:
            fs.fit_flux()
            dense = "taken"
        except DvError as e:
            dense = "refused: " + str(e).split(": ", 1)[-1]
        out = fs.fit_flux_groups()                                                    # warm-up
        t = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            out = fs.fit_flux_groups()
            t.append(time.perf_counter() - t0)
    finally:
        fs.close()
    t = np.array(t)
    sizes = out["fit_group_size"][out["fit_group"] == np.arange(2 * per_pass)]        # (one field: the label is the joint row)
    print(f"{dtype} crowded: one field of {F} px, 2 x {per_pass} rows in {len(sizes)} groups of {int(sizes.min())} .. {int(sizes.max())}; "
          f"the dense joint fit is {dense}")
    print(_row(f"{dtype} grouped joint fit", t, 1, 2 * per_pass))
    return {"rows": 2 * per_pass, "groups": int(len(sizes)), "largest": int(sizes.max()), "dense": dense,
            "fit_flux_groups_ms": [round(1e3 * x, 2) for x in t]}


def _row(label, t, fields, galaxies):
    med = float(np.median(t))
    return (f"{label:<22s} {fields / med:9.1f} fields/s {galaxies / med:10.0f} galaxies/s   median {1e3 * med:9.1f} ms   "
            f"spread {100 * (t.max() - t.min()) / med:5.1f} %   runs " + " ".join(f"{1e3 * x:.1f}" for x in t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=64)
    ap.add_argument("--size", type=int, default=259)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=8192)
    ap.add_argument("--dtype", choices=("both", "float32", "bf16"), default="both")
    ap.add_argument("--profile-one", action="store_true", help="warm up, one batched run, exit")
    ap.add_argument("--measure", action="store_true", help="time the batched form with and without the catalogue")
    ap.add_argument("--no-fields", action="store_true", help="time the batched form with and without the field downloads")
    ap.add_argument("--fit-flux", action="store_true", help="with --measure: time the catalogue with and without the joint flux fit")
    ap.add_argument("--fit-weights", action="store_true", help="the weighted fit")
    ap.add_argument("--fit-sky", type=int, choices=(0, 1), default=None, help="the fit with a sky of that order")
    ap.add_argument("--fit-nonneg", action="store_true", help="the non-negative fit")
    ap.add_argument("--fit-groups", action="store_true", help="with --fit-flux: also time the joint fit by blend groups")
    ap.add_argument("--crowded", type=int, default=0, metavar="ROWS_PER_PASS",
                    help="a leg of its own: the grouped joint fit of one field of two passes of that many clustered stamps")
    a = ap.parse_args()
    if a.fit_flux and not a.measure:
        ap.error("--fit-flux needs --measure: the fit belongs to the catalogue")
    if (a.fit_weights or a.fit_sky is not None or a.fit_nonneg) and not a.fit_flux:
        ap.error("--fit-weights, --fit-sky and --fit-nonneg need --fit-flux")
    if a.fit_groups and (not a.fit_flux or a.fit_sky is not None or a.fit_nonneg):
        ap.error("--fit-groups needs --fit-flux and goes with neither --fit-sky nor --fit-nonneg")
    if a.crowded and not (a.measure or a.no_fields):
        ap.error("--crowded is a leg of the --measure / --no-fields form")
    if a.crowded < 0:
        ap.error("--crowded takes the rows of a pass, at least 1")
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    fit = dict(fit_flux=True, fit_sky=a.fit_sky, fit_nonneg=a.fit_nonneg)
    if a.fit_weights:
        wrng = np.random.default_rng(1)
        fit["fit_weights"] = np.where(wrng.random(fields.shape) < 0.1, 0.0, wrng.uniform(0.5, 2.0, size=fields.shape))
    quiet = io.StringIO()                      # both classes print their progress
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat}
    print(f"{M} fields of {F} px, six bands; max_batch {a.max_batch}; reference mode")
    for dtype in (("float32", "bf16") if a.dtype == "both" else (a.dtype,)):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        core = net._core
        with redirect_stdout(quiet):
            _loop(net, fields[:2])                                                    # warm-up
            _batch(net, fields[:min(M, 8)])
            if a.profile_one and a.fit_flux:                                          # (the catalogue with the joint fit)
                _batch(net, fields, measure=True, blendedness=True, return_fields=not a.no_fields, fit_groups=a.fit_groups, **fit)
                core.engine.close()
                return
            if a.profile_one:
                _batch(net, fields)
                core.engine.close()
                return
        if a.measure or a.no_fields:
            cat = dict(measure=True, blendedness=True)
            forms = [("batch", {})]
            if a.measure:
                forms.append(("batch + catalogue", cat))
            if a.no_fields:
                forms.append(("batch, no fields", dict(return_fields=False)))
            if a.measure and a.no_fields:
                forms.append(("catalogue, no fields", dict(cat, return_fields=False)))
            pairs = []                         # (form with the fit, the same form without it)
            if a.fit_flux:
                forms.append(("catalogue + fit", dict(cat, **fit)))
                pairs.append(("catalogue + fit", "batch + catalogue"))
                if a.no_fields:
                    forms.append(("cat. + fit, no fields", dict(cat, return_fields=False, **fit)))
                    pairs.append(("cat. + fit, no fields", "catalogue, no fields"))
            if a.fit_groups:                   # (the grouped fit beside the dense one, and what it adds to the form without a fit)
                forms.append(("catalogue + grouped fit", dict(cat, fit_groups=True, **fit)))
                pairs += [("catalogue + grouped fit", "batch + catalogue"), ("catalogue + grouped fit", "catalogue + fit")]
                if a.no_fields:
                    forms.append(("cat. + gr. fit, no fields", dict(cat, return_fields=False, fit_groups=True, **fit)))
                    pairs += [("cat. + gr. fit, no fields", "catalogue, no fields"), ("cat. + gr. fit, no fields", "cat. + fit, no fields")]
            with redirect_stdout(quiet):
                for _, kw in forms[1:]:                                               # warm-up of the new stages
                    _batch(net, fields[:min(M, 8)], **{k: (v[:min(M, 8)] if k == "fit_weights" else v) for k, v in kw.items()})
            times = {label: [] for label, _ in forms}
            for _ in range(a.repeat):          # alternating; every run starts from the same seed counter
                for label, kw in forms:
                    core.seed_counter = 1000
                    with redirect_stdout(quiet):
                        t0 = time.perf_counter()
                        n, _ = _batch(net, fields, **kw)
                        times[label].append(time.perf_counter() - t0)
            for label, _ in forms:
                print(_row(f"{dtype} {label}", np.array(times[label]), M, n))
            med = {label: float(np.median(t)) for label, t in times.items()}
            for label, _ in forms[1:]:
                print(f"{dtype} {label} / batch: {med[label] / med['batch']:.3f} x")
            for with_fit, without in pairs:
                add = med[with_fit] - med[without]
                print(f"{dtype} {with_fit} - {without}: {1e3 * add:+.1f} ms per loop, {1e6 * add / max(n, 1):+.1f} us per galaxy "
                      f"({n} galaxies)")
            result[dtype] = {label: [round(1e3 * x, 2) for x in t] for label, t in times.items()}
            result[dtype]["galaxies"] = int(n)
            if a.crowded:
                result[dtype]["crowded"] = _crowded(core.engine, a.size, a.crowded, a.repeat, dtype)
            core.engine.close()
            continue
        tl, tb = [], []
        for _ in range(a.repeat):              # alternating; every run of either form starts from the same seed counter
            for fn, ts in ((_loop, tl), (_batch, tb)):
                core.seed_counter = 1000
                with redirect_stdout(quiet):
                    t0 = time.perf_counter()
                    n, passes = fn(net, fields)
                    ts.append(time.perf_counter() - t0)
                if fn is _loop:
                    nl, pl = n, passes
                else:
                    nb_, pb = n, passes
        tl, tb = np.array(tl), np.array(tb)
        print(_row(f"{dtype} loop", tl, M, nl))
        print(_row(f"{dtype} batch", tb, M, nb_))
        factor = float(np.median(tl) / np.median(tb))
        print(f"{dtype} loop / batch: {factor:.2f} x  (slowest batch {1e3 * tb.max():.1f} ms, fastest loop {1e3 * tl.min():.1f} ms)")
        lb = [loop_pass_bytes(F, d, g) for d, g in pl]
        bb = [batch_pass_bytes(M, d, g) for _, d, g in pb]
        print(f"{dtype} host link: loop {len(pl)} field passes, {np.mean(lb) / 1e6:.2f} MB per field and pass, "
              f"{sum(lb) / 1e6:.1f} MB in all; batch {len(pb)} passes over {[p[0] for p in pb]} fields, "
              f"{np.mean(bb) / 1e3:.1f} KB per pass ({np.mean(bb) / 1e3 / max(1, np.mean([p[0] for p in pb])):.2f} KB per "
              f"field and pass), {sum(bb) / 1e6:.3f} MB in all, plus {4 * M * F * F * NB * 8 / 1e6:.1f} MB once (fields up, three "
              f"result stacks down)")
        result[dtype] = {"loop_ms": [round(1e3 * x, 2) for x in tl], "batch_ms": [round(1e3 * x, 2) for x in tb],
                         "factor": round(factor, 3), "galaxies_loop": int(nl), "galaxies_batch": int(nb_),
                         "loop_field_passes": len(pl), "batch_passes": len(pb),
                         "loop_link_bytes": int(sum(lb)), "batch_link_bytes_between_passes": int(sum(bb)),
                         "batch_link_bytes_once": int(4 * M * F * F * NB * 8)}
        core.engine.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
