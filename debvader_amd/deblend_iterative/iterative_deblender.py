"""Iterative deblending of a field (reference: src/debvader/deblend_iterative/iterative_deblender.py).

The reference's loop restated line for line around this engine's DeblendField and its GPU detector
(debvader_amd.detect.detection.detect_objects: SExtractor's method in place of sep).  Its printed lines, the `mse` list,
the `list_idx` offset, the concatenated records and the residual of get_residual_field() on the latest step's records
are the reference's.  Three departures:
 - No detections: the reference's deblending_step then calls len(None) on the empty pass and raises TypeError; here it
   takes the "No more galaxies found" return that the reference's next line intends.  When that happens in the first
   pass, iterative_deblending records the mse of that pass (0: the residual is the field), prints "converged !" and
   returns None, the recarray it holds (the reference would fail on res_step["shifts"]).
 - optimise_positions=True: DeblendField.deblend_field keeps refusing it, so the step deblends with
   optimise_positions=False and then fits the positions of its rows against the field it deblended
   (DeblendField.optimise_positions, on the GPU) - the reference's fit.
 - Detection runs on the net's GPU context.

IterativeDeblendFieldBatch (engine-specific) runs the same loop for M fields that stay on the GPU:
one detector call and one network call per pass for all fields that are still iterating.
"""
import numpy as np

from debvader_amd.deblend.field_deblender import DeblendField, DeblendFieldBatch, batch_windows
from debvader_amd.detect.detection import _distances, detect_objects
from debvader_amd.training.metrics import mse


class IterativeDeblendField(DeblendField):
    def __init__(
        self,
        net,
        field_image,
        cutout_size=59,
        nb_of_bands=6,
        epistemic_uncertainty_estimation=False,
        normalise=False
    ):
        super().__init__(net, field_image, cutout_size, nb_of_bands, epistemic_uncertainty_estimation, normalise)

    def iterative_deblending(
        self,
        galaxy_distances_to_center=None,
        cutout_images=None,
        optimise_positions=False,
        epistemic_criterion=100.0,
        mse_criterion=100.0,
    ):
        """
        Do the iterative deblending of a scene
        paramters:
            galaxy_distances_to_center: distances of the galaxies to deblend from the center of the field. In pixels.
            cutout_images: stamps centered on the galaxies to deblend
            optimise_position: boolean to indicate if the user wants to optimise the position of the galaxies
            epistemic_criterion: cut for epistemic uncertainity to get rid of bad predictions
            mse_criterion: cut for mse_criterion to get rid of bad predictions
        """

        # do the first step of deblending
        field_image = self.field_image.copy()
        res_step = self.deblending_step(
            field_image,
            cutout_images=cutout_images,
            optimise_positions=optimise_positions,
            epistemic_criterion=epistemic_criterion,
            mse_criterion=mse_criterion,
        )
        res_deblend = res_step

        new_residual_field = self.get_residual_field()
        self.mse += [mse(self.field_image, new_residual_field)]
        if res_step is None:
            # departure: nothing was deblended in the first pass (the reference fails on res_step["shifts"] below)
            print("converged !")
            return self.res_deblend
        shifts_previous = []
        k = 1
        diff_mse = -1

        # Now iterate over
        while len(res_step["shifts"]) > len(shifts_previous):

            print(f"iteration {k}")
            shifts_previous = res_step["shifts"]

            prev_residual_field = new_residual_field

            # deblending step will run detection and deblending on the residual field
            res_step = self.deblending_step(
                prev_residual_field,
                cutout_images=None,
                optimise_positions=optimise_positions,
                mse_criterion=mse_criterion,
            )

            # compute the MSE after this iteration step
            new_residual_field = self.get_residual_field()
            self.mse += [mse(prev_residual_field, new_residual_field)]

            if res_step["list_idx"] is None:
                break

            res_deblend = np.concatenate([res_deblend, res_step])
            k += 1

            print(
                f"{sum(self.nb_of_deblended_galaxies)} galaxies found up to this step."
            )
            print(
                f"deta_mse = {diff_mse}, mse_iteration = "
                + str(self.mse[-1])
                + " and mse_previous_step = "
                + str(self.mse[-2])
            )

        print("converged !")

        self.res_deblend = res_deblend

        return self.res_deblend

    def deblending_step(
        self,
        field_image,
        cutout_images=None,
        optimise_positions=False,
        epistemic_criterion=100.0,
        mse_criterion=100.0,
    ):
        """
        One step of the iterative procedure called within iterative_procedure.

        paramters:
            field_image: image of the field to deblend
            cutout_images: stamps centered on the galaxies to deblend
            optimise_position: boolean to indicate if the user wants to optimise the position of the galaxies
            epistemic_criterion: cut for epistemic uncertainity to get rid of bad predictions
            mse_criterion: cut for mse_criterion to get rid of bad predictions
        """
        detection_k = detect_objects(field_image, ctx=self._ctx)

        res_step = self.deblend_field(
            field_image=field_image,
            galaxy_distances_to_center=detection_k,
            cutout_images=cutout_images,
            optimise_positions=False,
            epistemic_criterion=epistemic_criterion,
            mse_criterion=mse_criterion,
        )

        # departure: an empty pass (no detection, or none that fits a cutout) carries list_idx None
        if res_step["list_idx"] is None or len(res_step["list_idx"]) == 0:
            print("No more galaxies found")
            return self.res_deblend

        if optimise_positions:
            # departure: the reference's fit inside deblend_field, run on the rows of this pass against its field
            self.optimise_positions(res_step, field_image=field_image)

        res_step["list_idx"] += (
            sum(self.nb_of_deblended_galaxies) - self.nb_of_deblended_galaxies[-1]
        )

        print(f"Deblend {self.nb_of_deblended_galaxies[-1]} more galaxy(ies)")

        return res_step


class IterativeDeblendFieldBatch:
    """The loop of IterativeDeblendField for M fields of one size that are uploaded once and stay on the GPU
    (Engine.open_field_set): every pass is ONE detector call over the fields that are still iterating
    and ONE network call over their galaxies; the working residuals, the final residuals and the predicted fields never
    leave the device between passes - detections, mse_center and one mse per field do - and the composited fields come
    back once, at the end.

    Per field the loop is the reference's: pass 0 detects on the field, pass k on the residual of pass k - 1; galaxies
    whose window fits the field are deblended; the records of all passes are concatenated with the reference's list_idx
    offset.  Stamps are numbered over the active fields, field after field, and that number is a stamp's noise row; every
    pass that has stamps draws one seed.

    One deliberate departure from IterativeDeblendField: a pass in which a field has no detection, or none that fits a
    window, ends that field's loop and contributes nothing - no rows and no `mse` entry (the single-field class appends its
    previous records a second time, with an mse of 0).  The epistemic estimate and the position fit are not part of this
    loop; IterativeDeblendField has both."""

    COLUMNS = DeblendFieldBatch.ON_DEVICE_COLUMNS + [("iteration", "<i8")]
    DEFAULT_MAX_ITERATIONS_CUMULATIVE = 10

    def __init__(self, net, field_images, cutout_size=59, nb_of_bands=6, normalise=False):
        """
        parameters:
            net: network used to deblend the fields (it must run on the engine: load_deblender)
            field_images: the fields, shape (M, size, size, bands)
            cutout_size: size of the stamps
            nb_of_bands: number of filters in the images (at least 3: detection reads band 2)
            normalise: normalise the stamps before the network
        """
        core = getattr(net, "_core", None)
        if core is None or getattr(core, "engine", None) is None:
            raise ValueError("IterativeDeblendFieldBatch keeps the fields on the GPU and needs a net that runs on the engine "
                             "(debvader_amd.model.model.load_deblender); for any other net loop IterativeDeblendField over "
                             "the fields")
        if nb_of_bands < 3:
            raise ValueError(f"detection reads band 2 (r), these fields have {nb_of_bands} band(s); deblend given positions "
                             "with DeblendFieldBatch.deblend_fields instead")
        f = np.array(field_images, dtype=np.float64, copy=True, order="C")
        if f.ndim != 4 or f.shape[1] != f.shape[2] or f.shape[3] != nb_of_bands:
            raise ValueError(f"expected fields (M, F, F, {nb_of_bands}), got {f.shape}")
        self.net = net
        self.field_images = f
        self.nb_of_fields = f.shape[0]
        self.field_size = f.shape[1]
        self.cutout_size = cutout_size
        self.nb_of_bands = nb_of_bands
        self.normalise = normalise
        self.nb_of_detected_objects = []
        self.nb_of_deblended_galaxies = []
        self.res_deblend = None
        self.mse = [[] for _ in range(self.nb_of_fields)]
        self._fields = None
        self._no_fields = False
        self.sky_fit = None             # iterative_catalogue(fit_flux=True, fit_sky=...): the per-field arrays sky_coef, sky_cov,
                                        # sky_status, sky_npix of the joint fit, as DeblendFieldBatch holds them
        self.nonneg_fit = None          # ... (fit_nonneg=True): nonneg_iters and nonneg_status (M, bands)

    def _records(self, kept, dd, mse_center, passed, offset, iteration):
        n = len(kept)
        rec = np.recarray((n,), dtype=self.COLUMNS)
        rec["list_idx"] = np.asarray(kept, dtype=np.int64) + offset
        col = np.empty(n, dtype=object)
        for i in range(n):
            col[i] = np.array([0, 0])
        rec["shifts"] = col
        rec["galaxy_distances_to_center_x"] = dd[:, 0]
        rec["galaxy_distances_to_center_y"] = dd[:, 1]
        rec["mse_center"] = mse_center
        rec["passed_cuts"] = passed
        rec["iteration"] = iteration
        return rec

    @staticmethod
    def catalogue_columns(nb_of_bands, blendedness=False):
        """What iterative_catalogue(measure=True) appends behind COLUMNS: the catalogue of measure_stamps and `seen_before`;
        with blendedness=True also the columns of measure_blendedness and the residual statistic."""
        from debvader_amd.measure.measurement import blend_dtype, catalogue_dtype, residual_dtype

        cols = catalogue_dtype(nb_of_bands) + [("seen_before", "<i8")]
        return cols + (blend_dtype() + residual_dtype() if blendedness else [])

    @staticmethod
    def seen_before(iteration, centroids, match_radius):
        """For the rows of one field in recarray order: the index of the nearest row of an EARLIER pass whose centroid
        (field coordinates) lies within match_radius pixels, a tie going to the lowest index; -1 without one, and for
        every row of pass 0."""
        iteration = np.asarray(iteration)
        c = np.asarray(centroids, dtype=np.float64).reshape(-1, 2)
        out = np.full(len(c), -1, dtype=np.int64)
        for i in np.nonzero(iteration > 0)[0]:
            earlier = np.nonzero(iteration < iteration[i])[0]
            if not len(earlier):
                continue
            with np.errstate(invalid="ignore"):
                d2 = ((c[earlier] - c[i]) ** 2).sum(axis=1)
                d2 = np.where(d2 <= float(match_radius) ** 2, d2, np.inf)      # (a NaN centroid matches nothing)
            j = int(np.argmin(d2))                                             # (the first minimum: the lowest index)
            if np.isfinite(d2[j]):
                out[i] = earlier[j]
        return out

    def iterative_deblending(self, mse_criterion=100.0, mode="reference", max_iterations=None):
        """Run the loop on every field; returns a list of M recarrays (kept in self.res_deblend) with the columns of
        DeblendFieldBatch's on-device pass plus `iteration`, the pass a row was deblended in.  self.mse[m] has one entry
        per pass field m took.

        mode="reference": the reference's rule.  The residual after pass k is the ORIGINAL field minus the stamps of pass
            k only; a field goes on while a pass deblends more galaxies than the pass before it (the first counts against
            0).  mse[0] is the mse of the field against the residual of pass 0, mse[k] of residual k - 1 against residual k.
            max_iterations=None: no limit beside the rule.
        mode="cumulative" (engine-specific): every pass subtracts from the working residual, so pass k sees the field
            with everything found so far removed; a field goes on while a pass deblends at least one galaxy, for at most
            max_iterations passes (None: DEFAULT_MAX_ITERATIONS_CUMULATIVE = 10).
        In both modes get_residual_fields() is the field minus every deblended galaxy of every pass.

        iterative_catalogue() is this loop with the catalogue arguments behind these three; this method is that one with
        every one of them at its default, which makes the calls this method always made."""
        return self.iterative_catalogue(mse_criterion=mse_criterion, mode=mode, max_iterations=max_iterations)

    def iterative_catalogue(self, mse_criterion=100.0, mode="reference", max_iterations=None, measure=False,
                            blendedness=False, return_fields=True, band=2, sigma0=3.0, tol=1e-10, max_iter=200,
                            match_radius=2.0, fit_flux=False, fit_weights=None, fit_sky=None, fit_nonneg=False,
                            sky_sigma=None, min_pivot=1e-8, detect_shapes=False, detect_bands=None, detect_band_weights=None,
                            detect_clean=None, detect_weights=None, detect_noise=None, detect_filter="conv", detect_thresh=None, fit_groups=False):
        """iterative_deblending() with a catalogue measured on the GPU: the same loop, the same
        list of M recarrays (kept in self.res_deblend), self.mse and fields, and with every argument behind the first
        three left at its default the same calls.  The arguments are a method of their own because the parameter list of
        iterative_deblending is the reference's and is kept as it is.

        measure=True: every pass also measures its stamps where they lie on the GPU
            (FieldSet.deblend_pass_measure with band, sigma0, tol, max_iter as in measure_stamps) and the recarrays carry
            COLUMNS plus measurement.catalogue_dtype(bands) plus `seen_before`: for a row of pass k > 0 the index, in its
            field's recarray, of the nearest row of an earlier pass whose centroid - place + (row, col) in field pixels, the
            stamp's centre pixel for a row with status 3 - lies within match_radius pixels (a tie goes to the lowest
            index); -1 when there is none, and for every row of pass 0.  Every column shared with a measure=False run from
            the same seed counter, self.mse and the fields have the same bits.
        blendedness=True (needs measure=True): after the last pass one FieldSet.blend_sums call takes, per galaxy of
            every pass, the sums that need the complete set, and the recarrays also carry measurement.blend_dtype() -
            blend_model against the predicted mean fields of ALL passes, blend_data against the fields as given - and
            measurement.residual_dtype(): resid_sum, resid_sq, resid_mean, resid_rms of the final residual under the
            galaxy's weight.  In mode="reference" a galaxy that is deblended in several passes is in the predicted mean
            field several times, so its blendedness counts its own earlier copies as neighbours (seen_before finds
            them).  In mode="cumulative" the set keeps no copy of the fields as given: blend_data and blendedness_data are
            NaN on every row.
        return_fields=False: the three field-sized downloads at the end of the loop are skipped;
            get_residual_fields() and get_predicted_fields() then raise.
        fit_flux=True (needs measure=True): after the last pass ONE joint flux fit per field and band over the galaxies of
            EVERY pass, against the fields as given, on mean stamps that stayed on the GPU (FieldSet.keep_stamps and
            FieldSet.fit_flux): the model a bright galaxy got in pass 0 from a field that still held an
            undetected neighbour is refitted together with that neighbour's model of pass 1.  Every pass then takes the
            child sums, with or without blendedness.  Inside a field the unknowns stand in recarray order, so of two models
            that cannot be told apart - in mode="reference" a galaxy deblended again in a later pass - the later copy is
            dropped (fit_status 5, fit_scale 1) and the earlier detection is fitted.  The recarrays gain, behind the
            blendedness and residual columns, measurement.fit_flux_dtype(bands), with flux_fit = fit_scale * flux of the
            row's own pass.  fit_weights, fit_sky, fit_nonneg, sky_sigma and min_pivot mean what they mean in
            DeblendFieldBatch.deblend_fields and need fit_flux=True: fit_weights (M, F, F, bands) adds fit_chi2 and fit_npix
            and is refused beside sky_sigma, fit_sky = 0 or 1 adds measurement.fit_sky_dtype(bands) and self.sky_fit,
            fit_nonneg=True adds measurement.fit_nonneg_dtype(bands) and self.nonneg_fit - in that order.
        fit_groups=True (needs fit_flux=True): the joint fit is solved blend group by blend group, in place on the kept
            stamps (FieldSet.fit_flux_groups in place of FieldSet.fit_flux): a field may then hold any
            number of galaxies summed over its passes, 1024 per group.  The columns of the fit keep the bits of the fit
            without it wherever that one takes the field; behind them (and behind fit_chi2, fit_npix if weighted) the
            recarrays gain measurement.fit_groups_dtype(bands): fit_group, the smallest row of the galaxy's group in its
            field's recarray - the rows of all passes count, so a group may span passes -, and fit_group_size.  Together with
            fit_sky or fit_nonneg it is the ValueError of DeblendFieldBatch.deblend_fields.
        detect_weights (M, F, F) or (M, F, F, bands), of which band 2 is taken: every detection pass runs with a per-pixel
            noise map and a mask (FieldSet.set_detect_weights before the first pass): a pixel counts
            iff 0 < w < inf.  detect_noise "absolute" (the default with weights: inverse variances, the threshold in units
            of the pixel's sigma) or "relative" (relative weights, the threshold in units of globalrms), detect_filter "conv"
            or "matched", as in Context.scene_detect; both need detect_weights.  The fields themselves must stay finite,
            because the network reads them: fill the pixels under a bleed trail, a saturated core or a chip gap with finite
            values (the local sky, say) - the weights keep them out of every detection pass, whatever they hold.
        detect_thresh: the detection threshold of every pass (None: the detector's 1.5), with or without weights.
        detect_bands: a list of band numbers: every detection pass runs on the inverse-variance weighted combination of those
            bands of the working residual (FieldSet.set_detect_bands before the first pass) in place of
            band 2 alone, matched to the spectral shape detect_band_weights (None: flat).  detect_thresh is then in units of
            the combined pixel's own sigma.  detect_weights, if given, must be (M, F, F, bands): the planes of the selected
            bands are taken from it; three-dimensional weights are refused.  detect_noise and detect_filter mean what they mean
            without detect_bands; detect_filter then needs no weights.
            (The detect_* arguments are keywords: pass them, and fit_groups behind them, by name.)
        detect_shapes=True: every row carries the detection it was cut for, as the detector of its pass saw it
            (FieldSet.set_detect_objects before the first pass): behind all other columns DETECT_COLUMNS,
            det_npix, det_peak, det_flux, det_x, det_y, the box det_xmin .. det_ymax, the isophotal moments det_x2, det_y2,
            det_xy with det_a, det_b, det_theta, and det_flag (bit 1: the detection was split off a blend, 2: cut by the
            field's edge, 4: singular moments, 8: next to a pixel that does not count).  With or without measure; every other
            column, self.mse and the fields keep their bits.  detect_thresh must then be >= 0.
        detect_clean: True (clean_param 1.0) or a clean_param > 0: every detection pass is followed by SExtractor's cleaning
            pass (FieldSet.set_detect_clean before the first pass; sep's clean=True, which the
            reference's sep call leaves on): a detection that the wings of a brighter neighbour explain is merged into that
            neighbour and gets no stamp - in the first pass and in every residual pass.  None or False: no cleaning, the
            calls as they were.  detect_thresh must then be > 0.  With detect_shapes=True the det_ columns are the cleaned
            rows' and gain det_nmerged behind det_flag (1 + the detections merged into the row).

        mse_criterion, mode, max_iterations: as in iterative_deblending."""
        if mode not in ("reference", "cumulative"):
            raise ValueError(f"mode must be 'reference' (the reference's residual and stopping rule) or 'cumulative' "
                             f"(every pass subtracts from the working residual), got {mode!r}")
        cumulative = mode == "cumulative"
        if max_iterations is None and cumulative:
            max_iterations = self.DEFAULT_MAX_ITERATIONS_CUMULATIVE
        if max_iterations is not None and int(max_iterations) < 0:
            raise ValueError(f"max_iterations must be at least 0, got {max_iterations}")
        if blendedness and not measure:
            raise ValueError("blendedness=True needs measure=True: the weight of the sums is the measured galaxy's")
        if measure and not (np.isfinite(match_radius) and match_radius >= 0):
            raise ValueError(f"match_radius must be finite and at least 0, got {match_radius}")
        M, F, cs = self.nb_of_fields, self.field_size, self.cutout_size
        fit_flux, fit_nonneg, fit_groups = bool(fit_flux), bool(fit_nonneg), bool(fit_groups)
        if fit_flux and not measure:
            raise ValueError("fit_flux=True needs measure=True: the fit scales the measured fluxes of the passes")
        for given, name in ((fit_weights is not None, "fit_weights"), (fit_sky is not None, "fit_sky"),
                            (fit_nonneg, "fit_nonneg=True"), (sky_sigma is not None, "sky_sigma")):
            if given and not fit_flux:
                raise ValueError(f"{name} needs fit_flux=True: it belongs to the joint flux fit after the last pass")
        if fit_groups and not fit_flux:
            raise ValueError("fit_groups=True needs fit_flux=True: it solves the joint flux fit after the last pass blend group by "
                             "blend group, without a limit on the galaxies of a field")
        if fit_flux:
            from debvader_amd import engine as E
            from debvader_amd.measure import measurement as ms

            if fit_groups and (fit_sky is not None or fit_nonneg):
                raise ValueError(ms.GROUPS_TAKE_NO_SKY_NO_CONSTRAINT)
            if fit_sky is not None:
                E.sky_terms(fit_sky)
            if fit_weights is not None:
                if sky_sigma is not None:
                    raise ValueError(ms.WEIGHTS_CARRY_THE_NOISE)
                fit_weights = E.check_fit_weights(fit_weights, self.field_images.shape)
            if sky_sigma is not None:
                sky_sigma = ms.check_sky_sigma(sky_sigma, M, self.nb_of_bands)
            E.fit_flux_params(min_pivot)
        if detect_bands is None and detect_band_weights is not None:
            raise ValueError("detect_band_weights need detect_bands: they belong to the multi-band detector")
        if detect_bands is None and detect_weights is None and (detect_noise is not None or detect_filter != "conv"):
            raise ValueError("detect_noise and detect_filter need detect_weights: they belong to the weighted detector")
        detect_kw = {} if detect_thresh is None else {"thresh": float(detect_thresh)}
        detect_shapes = bool(detect_shapes)
        if detect_shapes and detect_thresh is not None and not float(detect_thresh) >= 0:
            raise ValueError(f"detect_shapes=True needs detect_thresh >= 0 (the moments weight every pixel above it), "
                             f"got {detect_thresh}")
        if isinstance(detect_clean, (bool, np.bool_)):
            detect_clean = 1.0 if detect_clean else None
        if detect_clean is not None:
            from debvader_amd import engine as E

            E.check_detect_clean(detect_clean, 1.5 if detect_thresh is None else detect_thresh, None)
            detect_clean = float(detect_clean)
        det_columns = self.DETECT_COLUMNS + (self.DETECT_CLEAN_COLUMNS if detect_clean is not None else [])
        shapes = [[] for _ in range(M)]      # detect_shapes: per field and pass, the detections of the kept rows
        if detect_bands is not None:
            from debvader_amd import engine as E

            detect_bands, detect_band_weights = E.check_detect_bands(self.nb_of_bands, detect_bands, detect_band_weights)
            if detect_weights is not None:
                detect_weights = np.asarray(detect_weights, dtype=np.float64)
                if detect_weights.shape != (M, F, F, self.nb_of_bands):
                    raise ValueError(f"with detect_bands the detect_weights must hold a plane per band, "
                                     f"{(M, F, F, self.nb_of_bands)}: got {detect_weights.shape}")
                detect_weights = np.ascontiguousarray(detect_weights[:, :, :, detect_bands])
            E.check_detect_band_planes((M, F, F, len(detect_bands)), detect_weights, None, detect_noise, detect_filter,
                                       1.5 if detect_thresh is None else detect_thresh)
        elif detect_weights is not None:
            from debvader_amd import engine as E

            detect_weights = np.asarray(detect_weights, dtype=np.float64)
            if detect_weights.ndim == 4 and detect_weights.shape[:3] == (M, F, F) and detect_weights.shape[3] > 2:
                detect_weights = detect_weights[:, :, :, 2]
            E.check_detect_weights((M, F, F), detect_weights, None, detect_noise, detect_filter,
                                   1.5 if detect_thresh is None else detect_thresh)
        take_sums = bool(blendedness) or fit_flux        # the passes that keep resident rows
        fit = None
        self.sky_fit = None
        self.nonneg_fit = None
        self._fields = None
        self._no_fields = not return_fields
        extra = [[] for _ in range(M)]       # measure=True: per field and pass, what joins the records at the end
        nrows = 0                            # stamps of the measured passes so far: the resident row of a pass's stamp 0
        core = self.net._core
        eng = core.engine
        self.nb_of_detected_objects = []
        self.nb_of_deblended_galaxies = []
        self.mse = [[] for _ in range(M)]
        steps = [[] for _ in range(M)]
        active = np.ones(M, dtype=bool)
        previous = [0] * M                   # galaxies the field's previous pass deblended
        total = [0] * M                      # ... and all its passes so far: the list_idx offset of the next one
        po = int((F - cs) / 2)
        fs = eng.open_field_set(self.field_images, cumulative=cumulative)
        try:
            if fit_flux:
                fs.keep_stamps()
            if detect_bands is not None:
                fs.set_detect_bands(detect_bands, band_weights=detect_band_weights, weights=detect_weights,
                                    noise=detect_noise, filter_type=detect_filter)
            elif detect_weights is not None:
                fs.set_detect_weights(detect_weights, noise=detect_noise, filter_type=detect_filter)
            if detect_shapes:
                fs.set_detect_objects(True)
            if detect_clean is not None:
                fs.set_detect_clean(True, detect_clean)
            k = 0
            while active.any() and (max_iterations is None or k < int(max_iterations)):
                det = fs.detect(active=active, **detect_kw)
                off = det["offsets"]
                dist = [_distances(det["x"][off[m]:off[m + 1]], det["y"][off[m]:off[m + 1]], F) if active[m]
                        else np.zeros((0, 2)) for m in range(M)]
                starts, field_ptr, kept, dd = batch_windows(F, dist, cs)
                N = len(starts)
                if N == 0:
                    active[:] = False       # an empty pass contributes nothing, for any field
                    break
                # where get_predicted_field puts a stamp: padded at int((F - cs) / 2) and shifted by the distance
                places = (po + dd).astype(np.int64)
                eng.set_normalise(bool(self.normalise))
                try:
                    if measure:
                        out = fs.deblend_pass_measure(starts, places, field_ptr, seed=core.next_seed(), band=band,
                                                      sigma0=sigma0, tol=tol, max_iter=max_iter, blend=take_sums)
                    else:
                        out = fs.deblend_pass(starts, places, field_ptr, seed=core.next_seed())
                finally:
                    eng.set_normalise(False)
                passed = ~(out["mse_center"] > mse_criterion)
                counts = [0] * M
                for m in range(M):
                    if not active[m]:
                        continue
                    lo, hi = int(field_ptr[m]), int(field_ptr[m + 1])
                    n = hi - lo
                    if n == 0:              # departure: this field's loop ends here, without rows or an mse entry
                        active[m] = False
                        continue
                    counts[m] = n
                    steps[m].append(self._records(kept[m], dd[lo:hi], out["mse_center"][lo:hi], passed[lo:hi], total[m], k))
                    if detect_shapes:
                        rows_m = int(off[m]) + np.asarray(kept[m], dtype=np.int64)
                        shapes[m].append({name: np.asarray(det[name[4:]])[rows_m] for name, _ in det_columns})
                    if measure:
                        e = {k: out[k][lo:hi] for k in ("flux", "flux_err", "shape", "iters", "status")}
                        e["places"] = np.asarray(places[lo:hi], dtype=np.float64)
                        if blendedness:
                            e.update(child=out["child"][lo:hi], npix=out["npix"][lo:hi])
                        if take_sums:
                            e.update(rows=np.arange(nrows + lo, nrows + hi))
                        extra[m].append(e)
                    self.mse[m].append(float(out["field_mse"][m]))
                    total[m] += n
                    if not cumulative and not n > previous[m]:
                        active[m] = False
                    previous[m] = n
                self.nb_of_detected_objects += [[len(d) for d in dist]]
                self.nb_of_deblended_galaxies += [counts]
                print(f"iteration {k}: {N} galaxy(ies) deblended in {sum(c > 0 for c in counts)} field(s), "
                      f"{int(active.sum())} field(s) go on")
                if measure:
                    nrows += N
                k += 1
            sums = fs.blend_sums(band=band) if blendedness else None
            if fit_groups:
                fit = fs.fit_flux_groups(data_fields=self.field_images if cumulative else None, weight_fields=fit_weights,
                                         min_pivot=min_pivot)
            elif fit_flux:
                fit = fs.fit_flux(data_fields=self.field_images if cumulative else None, weight_fields=fit_weights,
                                  sky_order=fit_sky, nonneg=fit_nonneg, min_pivot=min_pivot)
            if return_fields:
                self._fields = {"final": fs.read("final"), "mean": fs.read("mean"), "stddev": fs.read("stddev")}
        finally:
            fs.close()
        empty = np.recarray((0,), dtype=self.COLUMNS)
        self.res_deblend = [np.concatenate(s).view(np.recarray) if s else empty.copy() for s in steps]
        if measure:
            self.res_deblend = [self._with_catalogue(r, e, sums, bool(blendedness), match_radius)
                                for r, e in zip(self.res_deblend, extra)]
        if fit_flux:
            from debvader_amd import engine as E

            self.res_deblend = [self._with_fit(r, e, fit, m, sky_sigma, fit_weights is not None)
                                for m, (r, e) in enumerate(zip(self.res_deblend, extra))]
            if fit_sky is not None:
                self.sky_fit = {k: fit[k] for k in E.FIT_SKY_KEYS}
            if fit_nonneg:
                self.nonneg_fit = {k: fit[k] for k in E.FIT_NONNEG_FIELD_KEYS}
        if detect_shapes:
            self.res_deblend = [self._with_detections(r, d, det_columns) for r, d in zip(self.res_deblend, shapes)]
        return self.res_deblend

    # what iterative_catalogue(detect_shapes=True) appends behind every other column: the detection of the row's pass
    DETECT_COLUMNS = ([("det_npix", "<i4"), ("det_peak", "<f8"), ("det_flux", "<f8"), ("det_x", "<f8"), ("det_y", "<f8")]
                      + [("det_" + k, "<i4") for k in ("xmin", "xmax", "ymin", "ymax")]
                      + [("det_" + k, "<f8") for k in ("x2", "y2", "xy", "a", "b", "theta")] + [("det_flag", "<i4")])

    # ... and behind them with detect_clean
    DETECT_CLEAN_COLUMNS = [("det_nmerged", "<i4")]

    def _with_detections(self, rec, passes, columns=None):
        """The records of one field with DETECT_COLUMNS (or `columns`) behind them: per pass, the detector's rows of the
        kept stamps."""
        columns = self.DETECT_COLUMNS if columns is None else columns
        out = np.recarray((len(rec),), dtype=rec.dtype.descr + columns)
        for k in rec.dtype.names:
            out[k] = rec[k]
        for name, t in columns:
            out[name] = np.concatenate([d[name] for d in passes]) if passes else np.zeros(0, dtype=t)
        return out

    def _with_fit(self, rec, extra, fit, m, sky_sigma, weighted):
        """The catalogue of field m with the columns of the joint flux fit behind it: the rows of the fit joined by the
        resident row number, the per-field sky of field m, and what the host derives from them."""
        from debvader_amd import engine as E
        from debvader_amd.measure import measurement as ms

        nb = self.nb_of_bands
        rows = np.concatenate([e["rows"] for e in extra]).astype(np.int64) if extra else np.zeros(0, np.int64)
        sigma = None if sky_sigma is None else sky_sigma[m:m + 1]
        chi = dict(fit_chi2=fit["fit_chi2"][rows], fit_npix=fit["fit_npix"][rows]) if weighted else {}
        parts = [ms.fit_flux_records(*(fit[k][rows] for k in E.FIT_FLUX_KEYS), rec["flux"], sky_sigma=sigma, weighted=weighted,
                                     **chi)]
        if "fit_group" in fit:                 # (7y: no sky and no constraint beside it)
            parts.append(ms.fit_groups_records(fit["fit_group"][rows], fit["fit_group_size"][rows]))
        if "sky_coef" in fit:
            places = np.concatenate([e["places"] for e in extra]) if extra else np.zeros((0, 2))
            parts.append(ms.fit_sky_records(fit["sky_coef"][m:m + 1], fit["sky_cov"][m:m + 1], fit["sky_status"][m:m + 1],
                                            places, self.cutout_size, self.field_size, sky_sigma=sigma, weighted=weighted))
        if "fit_scale_free" in fit:
            parts.append(ms.fit_nonneg_records(*(fit[k][rows] for k in E.FIT_NONNEG_KEYS), rec["flux"]))
        out = np.recarray((len(rec),), dtype=rec.dtype.descr + [d for p in parts for d in p.dtype.descr])
        for p in [rec] + parts:
            for k in p.dtype.names:
                out[k] = p[k]
        return out

    def _with_catalogue(self, rec, extra, sums, blendedness, match_radius):
        """The records of one field with the catalogue columns behind them: the rows every pass measured, the end-of-loop
        sums joined to them by the resident row number, and seen_before."""
        from debvader_amd.measure.measurement import (STATUS_FAILED, blend_records, catalogue_records, residual_records)

        nb = self.nb_of_bands
        out = np.recarray((len(rec),), dtype=self.COLUMNS + self.catalogue_columns(nb, blendedness))
        for k in rec.dtype.names:
            out[k] = rec[k]

        def col(name, width):
            parts = [np.asarray(e[name]).reshape(len(e["status"]), *width) for e in extra]
            return np.concatenate(parts) if parts else np.zeros((0, *width))

        cat = catalogue_records(col("flux", (nb,)), col("flux_err", (nb,)), col("shape", (5,)),
                                col("iters", ()).astype(np.int32), col("status", ()).astype(np.int32))
        parts = [cat]
        # the centroid in field pixels; a failed measurement stands at the pixel its window is centred on
        centre = np.where((cat["status"] == STATUS_FAILED)[:, None], float(int(self.cutout_size / 2)),
                          np.stack([cat["row"], cat["col"]], axis=1))
        out["seen_before"] = self.seen_before(rec["iteration"], col("places", (2,)) + centre, match_radius)
        if blendedness:
            child, npix, rows = col("child", (2,)), col("npix", ()).astype(np.int32), col("rows", ()).astype(np.int64)
            s = np.asarray(sums, dtype=np.float64).reshape(-1, 4)[rows]
            parts += [blend_records(np.concatenate([child, s[:, :2]], axis=1), npix),
                      residual_records(child[:, 0], npix, s[:, 2], s[:, 3])]
        for p in parts:
            for k in p.dtype.names:
                out[k] = p[k]
        return out

    def _need_run(self):
        if self._fields is None:
            if getattr(self, "_no_fields", False):
                raise ValueError("iterative_catalogue() ran with return_fields=False: the fields were not read back; "
                                 "run it with return_fields=True")
            raise ValueError("no iterative_deblending() run yet")

    def get_residual_fields(self):
        """The fields minus every deblended galaxy of every pass, (M, F, F, bands)."""
        self._need_run()
        return self._fields["final"].copy()

    def get_predicted_fields(self):
        """{"predicted_mean_fields", "predicted_stddev_fields"}, each (M, F, F, bands): sums over all passes."""
        self._need_run()
        return {"predicted_mean_fields": self._fields["mean"].copy(),
                "predicted_stddev_fields": self._fields["stddev"].copy()}
