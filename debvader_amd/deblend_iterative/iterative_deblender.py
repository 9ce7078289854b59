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
"""
import numpy as np

from debvader_amd.deblend.field_deblender import DeblendField
from debvader_amd.detect.detection import detect_objects
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
