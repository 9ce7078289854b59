"""A catalogue of deblended galaxies - a flux and a shape per galaxy - for many small fields, on one GPU (DESIGN.md section
7j).  M synthetic six-band fields of F px as tools/fields_bench.py makes them (the section 7f workload: 1024 fields of 259 px),
detected once with detect_objects_batch, distances rounded to integers; then, alternating after a warm-up, --repeat times:

    (a) catalogue :  deblend_fields(d, on_device=True, measure=True, return_fields=False)   nothing field-sized comes back
    (b) both      :  deblend_fields(d, on_device=True, measure=True)                          catalogue and fields
    (c) fields    :  deblend_fields(d, on_device=True)                                        what the call was before
    (d) host      :  deblend_fields(d) on --host-fields fields (stamps to the host), then the numpy restatement of the
                     measurement (tests/measure_oracle.py) on every returned stamp: the only route to a catalogue before
                     the measurement existed.  Timed on the subset and EXTRAPOLATED to all fields by the ratio of stamps;
                     its two parts are reported separately.

Per leg: the median, the spread (max - min over the median) and every run.  GPU only; prints a table and one JSON line.

    python tools/measure_bench.py [--fields 1024] [--size 259] [--repeat 5] [--max-batch 8192] [--host-fields 16]

--profile-one: warm up, one fp32 catalogue-only call, exit (for a kernel trace).

--samples S (256 fields of 259 px is the section 7g workload): the Monte-Carlo catalogue instead -

    (a) mc catalogue :  deblend_fields(d, on_device=True, measure=True, return_fields=False, measure_samples=S)
    (b) mc composite :  deblend_fields(d, on_device=True, epistemic_uncertainty_estimation=True, epistemic_samples=S): the
                        nearest call before it, the same decodes folded per pixel and composited
    (c) route before :  infer_fields_keep, then S x infer_mc(cutouts, nsamples=1, seed=mc_seed + q), then S x scene_measure
                        on the downloaded sample stamps - the only route to these numbers before the stage existed.  Timed on
                        --host-fields fields and EXTRAPOLATED to all fields by the ratio of stamps.

    python tools/measure_bench.py --samples 100 --fields 256 [--repeat 5] [--host-fields 4]

With --profile-one: warm up, one fp32 call (a), exit.

--blend: what the blendedness stage costs in the catalogue-only call, on the same build and box -

    (a) catalogue       :  deblend_fields(d, on_device=True, measure=True, return_fields=False)
    (b) catalogue+blend :  the same with blendedness=True: the device-side mean field is composited, the child sums run
                           behind every chunk's measurement, the parent sums once a field is complete

    python tools/measure_bench.py --blend [--fields 1024] [--size 259] [--repeat 5]

--psf: what the PSF correction costs, on the same build and box, one 21-px double-Gaussian PSF per
field -

    (a) catalogue     :  deblend_fields(d, on_device=True, measure=True, return_fields=False): the call as it was
    (b) catalogue+psf :  the same with psf=(M, 21, 21): the PSFs are measured once, the re-Gaussianization runs behind every
                         chunk's measurement

    python tools/measure_bench.py --psf [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (b), exit.

--apertures: what the aperture photometry costs, on the same build and box, with the default radii
(3, 5, 8 px) and flux fractions (0.2, 0.5, 0.8) -

    (a) catalogue           :  deblend_fields(d, on_device=True, measure=True, return_fields=False): the call as it was
    (b) catalogue+apertures :  the same with apertures=(3, 5, 8): the circles, the Kron ellipse and the flux radii are taken
                               behind every chunk's measurement

    python tools/measure_bench.py --apertures [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (b), exit.

--aperture-data: what the same apertures on the observed field and the composited mean field cost, on
the same build and box, in --apertures' protocol -

    (a) catalogue                :  the catalogue-only call as above
    (b) catalogue+apertures      :  the same with apertures=(3, 5, 8): the baseline
    (c) catalogue+apertures+data :  the same with aperture_data=True: the mean field is composited on the device and the field
                                    sums are taken once a field's composite is complete

    python tools/measure_bench.py --aperture-data [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (c), exit.

--fit-flux: what the simultaneous flux fit costs, on the same build and box, in --aperture-data's
protocol (warm-up, then --repeat alternating runs, median and spread) -

    (a) catalogue          :  the catalogue-only call as above: the baseline
    (b) catalogue+fit-flux :  the same with fit_flux=True: the mean stamps are kept on the device and every field's amplitudes
                              are fitted to its observed pixels once its composite is complete

    python tools/measure_bench.py --fit-flux [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (b), exit.

--fit-weights: what per-pixel weights, masks and the chi-square add to the flux fit, in the same
protocol -

    (a) catalogue+fit-flux         :  the catalogue-only call with fit_flux=True: the baseline, to be compared with --fit-flux's
                                      leg (b) of the commit before - the unweighted path allocates and launches nothing new
    (b) catalogue+fit-flux+weights :  the same with fit_weights: uniform(0.25, 4) inverse variances with a tenth of the pixels
                                      masked, as large as the fields and uploaded beside them

    python tools/measure_bench.py --fit-weights [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (b), exit.

--fit-sky ORDER: what a sky background fitted jointly (ORDER 0: a constant, 1: a plane) adds to the flux
fit, in the same protocol, four legs alternating -

    (a) catalogue+fit-flux             :  the catalogue-only call with fit_flux=True, to be compared with --fit-weights' leg (a)
                                          of the commit before: without fit_sky nothing new is allocated or launched
    (b) catalogue+fit-flux+sky         :  the same with fit_sky=ORDER
    (c) catalogue+fit-flux+weights     :  leg (b) of --fit-weights, to be compared with it likewise
    (d) catalogue+fit-flux+weights+sky :  the same with fit_sky=ORDER

    python tools/measure_bench.py --fit-sky 1 [--fields 1024] [--size 259] [--repeat 5]

With --profile-one: warm up, one fp32 call (d), exit.

--fit-nonneg: what the constraint a_i >= 0 adds to the flux fit, in the same protocol, four legs
alternating -

    (a) catalogue+fit-flux            :  leg (a) of --fit-sky, to be compared with it on the commit before: without fit_nonneg
                                         nothing new is allocated or launched
    (b) catalogue+fit-flux+nonneg     :  the same with fit_nonneg=True: the active-set kernel in place of the solve
    (c) catalogue+fit-flux+sky        :  leg (b) of --fit-sky 1, to be compared with it likewise
    (d) catalogue+fit-flux+sky+nonneg :  the same with fit_nonneg=True

    python tools/measure_bench.py --fit-nonneg [--fields 1024] [--size 259] [--repeat 5]

It also prints how many (field, band) systems took 0, 1, 2, ... factorisations (nonneg_iters) in legs (b) and (d), and how many
galaxy-bands were clamped.  With --profile-one: warm up, one fp32 call (d), exit.

--fit-groups: the flux fit by blend groups, in the same protocol, two legs:

    (a) catalogue+fit-flux / catalogue+fit-flux+groups :  the catalogue-only call with fit_flux=True, dense and then with
                                                          fit_groups=True, alternating in one process; it also prints the
                                                          histogram of fit_group_size
    (b) one field of --tile pixels (4096) with --tile-stamps (20000) stamps of 31 pixels in 3 bands, the places a seeded uniform
        draw, through Context.scene_fit_flux_groups: time alone - the dense call refuses this field.  A draw with a group above
        1024 is thinned (every second member of such a group leaves, until none is left) and the run says so; the histogram of
        the group sizes is printed.

    python tools/measure_bench.py --fit-groups [--fields 1024] [--size 259] [--repeat 5] [--tile 4096] [--tile-stamps 20000]

--moments-data: what the adaptive moments on the observed field with the neighbours subtracted cost in
the catalogue-only call, on the same build and box, in --blend's protocol -

    (a) catalogue              :  deblend_fields(d, on_device=True, measure=True, return_fields=False): the call as it was
    (b) catalogue+moments-data :  the same with moments_data=True: the mean stamps are kept on the device, the mean field is
                                  composited there, and every galaxy's child image is measured once its field is complete

    python tools/measure_bench.py --moments-data [--fields 1024] [--size 259] [--repeat 5]

It also prints the histograms of status and status_data and the mean ratio iters_data / iters over the galaxies converged in
both.  With --profile-one: warm up, one fp32 call (b), exit.

The cost is reported, not gated.
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
from debvader_amd.deblend.field_deblender import DeblendFieldBatch  # noqa: E402
from debvader_amd.detect.detection import detect_objects_batch  # noqa: E402
from debvader_amd.model import model  # noqa: E402
from tests import measure_oracle  # noqa: E402
from tools.fields_bench import ARCH, _field, _row  # noqa: E402


def _device(net, fields, dists, **kw):
    return sum(len(r) for r in DeblendFieldBatch(net, fields).deblend_fields(dists, on_device=True, **kw))


def _host(net, fields, dists, parts):
    t0 = time.perf_counter()
    res = DeblendFieldBatch(net, fields).deblend_fields(dists)
    t1 = time.perf_counter()
    n = 0
    for rec in res:
        if len(rec):
            mean, std = np.stack(list(rec["output_images_mean"])), np.stack(list(rec["output_images_stddev"]))
            measure_oracle.measure(mean, std)
            n += len(rec)
    parts.append((t1 - t0, time.perf_counter() - t1))
    return n


def _route_before(net, fields, dists, S):
    """Route (c): every sample stamp visits the host and goes up again to be measured"""
    from debvader_amd.deblend.field_deblender import batch_windows

    eng = net._core.engine
    starts, field_ptr, _, _ = batch_windows(fields.shape[1], dists, ARCH["input_shape"][0])
    seed, mc_seed = net._core.next_seed(), net._core.next_seed()
    cut = eng.infer_fields_keep(fields, starts, field_ptr, seed=seed)["cutouts"].astype(np.float32)
    for q in range(S):
        eng.scene_measure(eng.infer_mc(cut, 1, mc_seed + q)[0])
    return len(starts)


def main_samples(a):
    rng = np.random.default_rng(0)
    F, M, S = a.size, a.fields, a.samples
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    quiet = io.StringIO()
    Mh = min(M, a.host_fields)
    result = {"fields": M, "F": F, "samples": S, "max_batch": a.max_batch, "repeat": a.repeat, "route_before_fields": Mh}
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; {S} Monte-Carlo samples; "
                  f"max_batch {a.max_batch}")
        legs = {"mc catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False, measure_samples=S),
                "mc composite": lambda: _device(net, fields, dists, epistemic_uncertainty_estimation=True, epistemic_samples=S)}
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                legs["mc catalogue"]()
                net._core.engine.close()
                return
            _route_before(net, fields[:1], dists[:1], 2)
            times = {k: [] for k in legs}
            before_t, n, nh = [], 0, 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                nh = _route_before(net, fields[:Mh], dists[:Mh], S)
                before_t.append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n, "route_before_stamps": nh}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace(" ", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        tb = np.array(before_t)
        print(_row(f"{dtype} route before ({Mh} fields)", tb, nh, Mh))
        scale = n / max(nh, 1)
        ta, tc = (float(np.median(times[k])) for k in ("mc catalogue", "mc composite"))
        ext = float(np.median(tb)) * scale
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        print(f"{dtype} route before EXTRAPOLATED to {M} fields ({n} stamps, x {scale:.1f}): {1e3 * ext:.0f} ms")
        print(f"{dtype} mc catalogue / mc composite {ta / tc:.3f}; extrapolated route before / mc catalogue {ext / ta:.1f} "
              f"(spreads {spread(times['mc catalogue']):.3f} and {spread(tb):.3f})")
        result[dtype].update(route_before_ms=[round(1e3 * x, 2) for x in tb], route_before_extrapolated_ms=round(1e3 * ext, 1))
        net._core.engine.close()
    print(json.dumps(result))


def main_blend(a):
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    quiet = io.StringIO()
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "blend": True}
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; max_batch {a.max_batch}")
        legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False),
                "catalogue+blend": lambda: _device(net, fields, dists, measure=True, return_fields=False, blendedness=True)}
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            times = {k: [] for k in legs}
            n = 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace("+", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        tc, tb = (float(np.median(times[k])) for k in legs)
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        print(f"{dtype} catalogue+blend / catalogue {tb / tc:.3f}: {1e3 * (tb - tc):+.1f} ms for {n} galaxies "
              f"(spreads {spread(times['catalogue']):.3f} and {spread(times['catalogue+blend']):.3f})")
        net._core.engine.close()
    print(json.dumps(result))


def main_fit_flux(a):
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    quiet = io.StringIO()
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "fit_flux": True, "fit_weights": bool(a.fit_weights),
              "fit_sky": a.fit_sky, "fit_nonneg": bool(a.fit_nonneg), "fit_groups": bool(a.fit_groups)}
    weights = None
    if a.fit_weights or a.fit_sky is not None:
        w16 = rng.uniform(0.25, 4.0, size=base.shape)
        w16[rng.random(base.shape) < 0.1] = 0.0
        weights = np.ascontiguousarray(w16[np.arange(M) % 16])
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections, at most {max(len(d) for d in dists)} "
                  f"per field; max_batch {a.max_batch}")
        seen, nonneg, sizes = [], {}, []

        def with_fit(**kw):
            batch = DeblendFieldBatch(net, fields)
            res = batch.deblend_fields(dists, on_device=True, measure=True, return_fields=False, fit_flux=True, **kw)
            seen[:] = [np.concatenate([r["fit_status"] for r in res]), np.concatenate([r["fit_independence"] for r in res])]
            if kw.get("fit_groups"):
                sizes[:] = [np.concatenate([r["fit_group_size"][r["fit_group"] == np.arange(len(r))] for r in res])]
            if batch.nonneg_fit is not None:      # per leg (keyed by its sky): the iterations and the clamped galaxy-bands
                nonneg[kw.get("fit_sky")] = (np.bincount(batch.nonneg_fit["nonneg_iters"].ravel()).tolist(),
                                             int(batch.nonneg_fit["nonneg_status"].sum()),
                                             int(sum(r["fit_clamped"].sum() for r in res)), int(seen[0].size))
            return sum(len(r) for r in res)

        if a.fit_groups:
            legs = {"catalogue+fit-flux": with_fit, "catalogue+fit-flux+groups": lambda: with_fit(fit_groups=True)}
        elif a.fit_nonneg:
            legs = {"catalogue+fit-flux": with_fit, "catalogue+fit-flux+nonneg": lambda: with_fit(fit_nonneg=True),
                    "catalogue+fit-flux+sky": lambda: with_fit(fit_sky=1),
                    "catalogue+fit-flux+sky+nonneg": lambda: with_fit(fit_sky=1, fit_nonneg=True)}
        elif a.fit_sky is not None:
            legs = {"catalogue+fit-flux": with_fit, "catalogue+fit-flux+sky": lambda: with_fit(fit_sky=a.fit_sky),
                    "catalogue+fit-flux+weights": lambda: with_fit(fit_weights=weights),
                    "catalogue+fit-flux+weights+sky": lambda: with_fit(fit_weights=weights, fit_sky=a.fit_sky)}
        elif a.fit_weights:
            legs = {"catalogue+fit-flux": with_fit, "catalogue+fit-flux+weights": lambda: with_fit(fit_weights=weights)}
        else:
            legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False),
                    "catalogue+fit-flux": with_fit}
        names = list(legs)
        last = names[-1]
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                legs[last]()
                net._core.engine.close()
                return
            times = {k: [] for k in legs}
            n = 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        counts = np.bincount(seen[0].ravel(), minlength=6).tolist()
        result[dtype] = {"stamps": n, "fit_status": counts}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace("+", "_").replace("-", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        ind = seen[1][np.isfinite(seen[1])]
        for first, second in zip(names[0::2], names[1::2]):       # (every pair: a leg and the leg that adds to it)
            tc, tf = float(np.median(times[first])), float(np.median(times[second]))
            print(f"{dtype} {second} / {first} {tf / tc:.3f}: {1e3 * (tf - tc):+.1f} ms for {n} galaxies, "
                  f"{1e6 * (tf - tc) / max(n, 1):.2f} us per galaxy (spreads {spread(times[first]):.3f} and "
                  f"{spread(times[second]):.3f}); fit_status 0 .. 5 over galaxies x bands: {counts}; median "
                  f"fit_independence {float(np.median(ind)) if ind.size else float('nan'):.3f}")
        for sky, (iters, capped, clamped, total) in nonneg.items():
            print(f"{dtype} fit_nonneg{'' if sky is None else f' with fit_sky={sky}'}: (field, band) systems by nonneg_iters 0, 1, 2, ... "
                  f"{iters}; {capped} reached max_iter; {clamped} of {total} galaxy-bands clamped")
            result[dtype]["nonneg_iters" + ("" if sky is None else "_sky")] = iters
        if sizes:
            hist = np.bincount(sizes[0]).tolist()
            print(f"{dtype} fit_groups: {len(sizes[0])} blend groups; groups by fit_group_size 0, 1, 2, ... {hist}")
            result[dtype]["group_sizes"] = hist
        net._core.engine.close()
    if a.fit_groups:
        result["tile"] = main_fit_groups_tile(a)
    print(json.dumps(result))


def main_fit_groups_tile(a):
    """Leg (b) of --fit-groups: one large field beyond the dense limit, host arrays in, time alone"""
    from debvader_amd import engine as E
    from tests import fit_flux_oracle as fo

    F, n, cs, nb = a.tile, a.tile_stamps, 31, 3
    rng = np.random.default_rng(11)
    places = rng.integers(-cs // 2, F - cs // 2, size=(n, 2)).astype(np.int32)
    ctx = E.default_context()
    thinned = 0
    while True:                                  # thin the groups the fit would refuse: every second member leaves
        g = ctx.scene_fit_groups(places, cs, F)
        big = g["fit_group_size"] > E.FIT_FLUX_MAX_N
        if not big.any():
            break
        drop = np.nonzero(big)[0][::2]
        thinned += len(drop)
        places = np.delete(places, drop, axis=0)
    n = len(places)
    roots = g["fit_group"] == np.arange(n)
    sizes = g["fit_group_size"][roots]
    edges = [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, 1025]
    hist = np.histogram(sizes, bins=edges)[0].tolist()
    blobs = np.stack([fo.elliptical_gaussian(cs, (rng.uniform(3, 8), 0.0, rng.uniform(3, 8))) for _ in range(64)])
    stamps = (blobs[rng.integers(0, 64, n)][..., None] * rng.uniform(0.5, 2.0, size=(n, 1, 1, nb))).astype(np.float32)
    data = rng.normal(0.0, 0.05, size=(1, F, F, nb))
    ctx.scene_fit_flux_groups(stamps, places, data)                  # warm-up
    t = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        out = ctx.scene_fit_flux_groups(stamps, places, data)
        t.append(time.perf_counter() - t0)
    t = np.array(t)
    print(f"tile of {F} px, {n} stamps of {cs} px x {nb} bands ({thinned} thinned out of groups above {E.FIT_FLUX_MAX_N}): "
          f"{int(roots.sum())} blend groups, the largest {int(sizes.max())}; groups by size [1, 2, 3-4, 5-8, ..., 513-1024]: {hist}")
    print(f"scene_fit_flux_groups, host arrays in and out: median {1e3 * np.median(t):.1f} ms, min {1e3 * t.min():.1f}, max "
          f"{1e3 * t.max():.1f} over {a.repeat} runs; fit_status 0 .. 5: {np.bincount(out['fit_status'].ravel(), minlength=6).tolist()}")
    return {"F": F, "stamps": n, "thinned": thinned, "groups": int(roots.sum()), "largest": int(sizes.max()), "size_hist": hist,
            "ms": [round(1e3 * x, 2) for x in t]}


def _bench_psfs(M, ps=21):
    """One PSF per field: 0.85 core + 0.15 wing (the wing's covariance 4x the core's), core sigma 1.2 - 1.6 px, a little
    elliptical, off the pixel centre"""
    rng = np.random.default_rng(5)
    r = np.arange(ps, dtype=np.float64)[:, None] - (ps - 1) / 2.0
    c = np.arange(ps, dtype=np.float64)[None, :] - (ps - 1) / 2.0
    out = np.zeros((M, ps, ps))
    for m in range(M):
        sig, e1, e2 = rng.uniform(1.2, 1.6), rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08)
        t = 2.0 * sig * sig / np.sqrt(1.0 - e1 * e1 - e2 * e2)
        Mrr, Mrc, Mcc = 0.5 * t * (1.0 - e1), 0.5 * t * e2, 0.5 * t * (1.0 + e1)
        dr, dc = r - rng.uniform(-0.5, 0.5), c - rng.uniform(-0.5, 0.5)
        for w, k in ((0.85, 1.0), (0.15, 4.0)):
            det = k * k * (Mrr * Mcc - Mrc * Mrc)
            out[m] += w / (2.0 * np.pi * np.sqrt(det)) * np.exp(-0.5 * k * (Mcc * dr * dr - 2.0 * Mrc * dr * dc + Mrr * dc * dc) / det)
    return out


def main_psf(a):
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    psf = _bench_psfs(M)
    quiet = io.StringIO()
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "psf": int(psf.shape[1])}
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; one {psf.shape[1]}-px PSF per field; "
                  f"max_batch {a.max_batch}")
        status = []

        def with_psf():
            res = DeblendFieldBatch(net, fields).deblend_fields(dists, on_device=True, measure=True, return_fields=False, psf=psf)
            status[:] = [np.concatenate([r["regauss_status"] for r in res])]
            return sum(len(r) for r in res)

        legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False), "catalogue+psf": with_psf}
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                legs["catalogue+psf"]()
                net._core.engine.close()
                return
            times = {k: [] for k in legs}
            n = 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n, "regauss_status": np.bincount(status[0], minlength=7).tolist()}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace("+", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        tc, tp = (float(np.median(times[k])) for k in legs)
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        print(f"{dtype} catalogue+psf / catalogue {tp / tc:.3f}: {1e3 * (tp - tc):+.1f} ms for {n} galaxies, "
              f"{1e6 * (tp - tc) / max(n, 1):.2f} us per galaxy (spreads {spread(times['catalogue']):.3f} and "
              f"{spread(times['catalogue+psf']):.3f}); regauss_status 0 .. 6: {result[dtype]['regauss_status']}")
        net._core.engine.close()
    print(json.dumps(result))


def main_apertures(a, data=False):
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    radii = (3.0, 5.0, 8.0)
    quiet = io.StringIO()
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "apertures": list(radii)}
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; apertures {radii} px, flux "
                  f"fractions 0.2 / 0.5 / 0.8; max_batch {a.max_batch}")
        seen = []

        def with_apertures(**kw):
            res = DeblendFieldBatch(net, fields).deblend_fields(dists, on_device=True, measure=True, return_fields=False,
                                                                apertures=radii, **kw)
            seen[:] = [np.concatenate([r["aper_status"] for r in res]), np.concatenate([r["aper_flags"] for r in res])]
            if kw:
                seen.append(np.concatenate([r["aper_data_flags"] for r in res]))
            return sum(len(r) for r in res)

        legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False),
                "catalogue+apertures": with_apertures}
        if data:
            legs["catalogue+apertures+data"] = lambda: with_apertures(aperture_data=True)
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                list(legs.values())[-1]()
                net._core.engine.close()
                return
            times = {k: [] for k in legs}
            n = 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n, "aper_status": np.bincount(seen[0], minlength=8).tolist(),
                         "kron_min_decides": int(np.count_nonzero(seen[1] & (1 << 10))),
                         "truncated": int(np.count_nonzero(seen[1] & 0x3ff))}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace("+", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        tc, tp = (float(np.median(times[k])) for k in list(legs)[:2])
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        if data:
            td = float(np.median(times["catalogue+apertures+data"]))
            result[dtype]["field_truncated"] = int(np.count_nonzero(seen[2]))
            print(f"{dtype} catalogue+apertures+data / catalogue+apertures {td / tp:.3f}: {1e3 * (td - tp):+.1f} ms for {n} "
                  f"galaxies, {1e6 * (td - tp) / max(n, 1):.2f} us per galaxy (spread "
                  f"{spread(times['catalogue+apertures+data']):.3f}); the field edge truncates an aperture of "
                  f"{result[dtype]['field_truncated']} galaxies")
        print(f"{dtype} catalogue+apertures / catalogue {tp / tc:.3f}: {1e3 * (tp - tc):+.1f} ms for {n} galaxies, "
              f"{1e6 * (tp - tc) / max(n, 1):.2f} us per galaxy (spreads {spread(times['catalogue']):.3f} and "
              f"{spread(times['catalogue+apertures']):.3f}); aper_status 0 .. 7: {result[dtype]['aper_status']}, kron_min decides "
              f"{result[dtype]['kron_min_decides']}, truncated {result[dtype]['truncated']}")
        net._core.engine.close()
    print(json.dumps(result))


def main_moments_data(a):
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    quiet = io.StringIO()
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "moments_data": True}
    dists = None
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; max_batch {a.max_batch}")
        seen = []

        def with_moments():
            res = DeblendFieldBatch(net, fields).deblend_fields(dists, on_device=True, measure=True, return_fields=False,
                                                                moments_data=True)
            seen[:] = [np.concatenate([r[k] for r in res]) for k in ("status", "status_data", "iters", "iters_data")]
            return sum(len(r) for r in res)

        legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False),
                "catalogue+moments-data": with_moments}
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                with_moments()
                net._core.engine.close()
                return
            times = {k: [] for k in legs}
            n = 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
        both = (seen[0] == 0) & (seen[1] == 0)
        ratio = float(np.mean(seen[3][both] / seen[2][both])) if both.any() else float("nan")
        result[dtype] = {"stamps": n, "status": np.bincount(seen[0], minlength=4).tolist(),
                         "status_data": np.bincount(seen[1], minlength=4).tolist(), "converged_in_both": int(both.sum()),
                         "mean_iters": round(float(np.mean(seen[2])), 2), "mean_iters_data": round(float(np.mean(seen[3])), 2),
                         "mean_iters_data_over_iters": round(ratio, 3)}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k.replace("+", "_").replace("-", "_") + "_ms"] = [round(1e3 * x, 2) for x in t]
        tc, tm = (float(np.median(times[k])) for k in legs)
        spread = lambda t: float((np.max(t) - np.min(t)) / np.median(t))
        print(f"{dtype} catalogue+moments-data / catalogue {tm / tc:.3f}: {1e3 * (tm - tc):+.1f} ms for {n} galaxies, "
              f"{1e6 * (tm - tc) / max(n, 1):.2f} us per galaxy (spreads {spread(times['catalogue']):.3f} and "
              f"{spread(times['catalogue+moments-data']):.3f}); status 0 .. 3 {result[dtype]['status']}, status_data "
              f"{result[dtype]['status_data']}; iterations per galaxy {result[dtype]['mean_iters']} on the model and "
              f"{result[dtype]['mean_iters_data']} on the data, mean iters_data / iters over the {int(both.sum())} converged in "
              f"both {ratio:.3f}")
        net._core.engine.close()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", type=int, default=1024)
    ap.add_argument("--size", type=int, default=259)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=8192)
    ap.add_argument("--host-fields", type=int, default=16)
    ap.add_argument("--dtypes", default="float32,bf16")
    ap.add_argument("--profile-one", action="store_true")
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--blend", action="store_true")
    ap.add_argument("--psf", action="store_true")
    ap.add_argument("--apertures", action="store_true")
    ap.add_argument("--aperture-data", action="store_true")
    ap.add_argument("--fit-flux", action="store_true")
    ap.add_argument("--fit-weights", action="store_true")
    ap.add_argument("--fit-sky", type=int, choices=(0, 1), default=None, metavar="ORDER")
    ap.add_argument("--fit-nonneg", action="store_true")
    ap.add_argument("--fit-groups", action="store_true")
    ap.add_argument("--moments-data", action="store_true")
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--tile-stamps", type=int, default=20000)
    a = ap.parse_args()
    if a.fit_flux or a.fit_weights or a.fit_sky is not None or a.fit_nonneg or a.fit_groups:
        return main_fit_flux(a)
    if a.moments_data:
        return main_moments_data(a)
    if a.aperture_data:
        return main_apertures(a, data=True)
    if a.apertures:
        return main_apertures(a)
    if a.psf:
        return main_psf(a)
    if a.blend:
        return main_blend(a)
    if a.samples > 0:
        return main_samples(a)
    rng = np.random.default_rng(0)
    F, M = a.size, a.fields
    base = np.stack([_field(rng, F, int(round(40 * (F / 259) ** 2))) for _ in range(16)])
    fields = np.ascontiguousarray(base[np.arange(M) % 16])
    quiet = io.StringIO()                      # the classes print the reference's notes about dropped galaxies
    result = {"fields": M, "F": F, "max_batch": a.max_batch, "repeat": a.repeat, "host_fields": min(M, a.host_fields)}
    dists = None
    Mh = min(M, a.host_fields)
    for dtype in a.dtypes.split(","):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=a.max_batch, seed=1, dtype=dtype)
        if dists is None:
            dists = detect_objects_batch(fields, ctx=net._core.ctx)
            dists = [np.round(np.asarray(d, dtype=np.float64).reshape(-1, 2)) for d in dists]
            print(f"{M} fields of {F} px, six bands; {sum(len(d) for d in dists)} detections; max_batch {a.max_batch}")
        legs = {"catalogue": lambda: _device(net, fields, dists, measure=True, return_fields=False),
                "both": lambda: _device(net, fields, dists, measure=True),
                "fields": lambda: _device(net, fields, dists)}
        parts = []
        with redirect_stdout(quiet):
            for fn in legs.values():           # warm-up
                fn()
            if a.profile_one:
                legs["catalogue"]()
                net._core.engine.close()
                return
            _host(net, fields[:2], dists[:2], [])
            times = {k: [] for k in legs}
            host_t, n, nh = [], 0, 0
            for _ in range(a.repeat):
                for k, fn in legs.items():
                    t0 = time.perf_counter()
                    n = fn()
                    times[k].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                nh = _host(net, fields[:Mh], dists[:Mh], parts)
                host_t.append(time.perf_counter() - t0)
        result[dtype] = {"stamps": n, "host_stamps": nh}
        for k in legs:
            t = np.array(times[k])
            print(_row(f"{dtype} {k}", t, n, M))
            result[dtype][k + "_ms"] = [round(1e3 * x, 2) for x in t]
        th = np.array(host_t)
        print(_row(f"{dtype} host route ({Mh} fields)", th, nh, Mh))
        scale = n / max(nh, 1)
        pd, pm = np.median([p[0] for p in parts]), np.median([p[1] for p in parts])
        print(f"{dtype} host route EXTRAPOLATED to {M} fields ({n} stamps, x {scale:.1f}): {1e3 * np.median(th) * scale:.0f} ms "
              f"(deblend_fields {1e3 * pd * scale:.0f} ms + numpy measurement {1e3 * pm * scale:.0f} ms)")
        tc, tb, tf = (float(np.median(times[k])) for k in ("catalogue", "both", "fields"))
        print(f"{dtype} catalogue / fields {tc / tf:.3f}, both / fields {tb / tf:.3f}, extrapolated host route / catalogue "
              f"{np.median(th) * scale / tc:.1f}")
        result[dtype].update(host_ms=[round(1e3 * x, 2) for x in th], host_extrapolated_ms=round(1e3 * float(np.median(th)) * scale, 1),
                             host_deblend_ms=round(1e3 * float(pd), 2), host_numpy_ms=round(1e3 * float(pm), 2))
        net._core.engine.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
