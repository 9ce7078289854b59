"""numpy float64 restatement of the end-of-loop sums of a resident field set (dv_field_set_blend,
blend_set_kernel in csrc/blend.hip), for the tests.  Per resident row, over the stamp pixels that lie inside the field, in
plain raster order and with the weight g and the eligibility rule of tests/blend_oracle.py: Bm = sum g mean, Bd = sum g base,
R1 = sum g final, R2 = sum g (final final); also the scale of each sum's rounding error, sum g |x| (sum g x^2 for R2)."""
import numpy as np

from tests import blend_oracle as bo


def sums(cs, shape, status, places, field, mean, base, final, band=2, total=bo.raster_sum):
    """{"sums" (n, 4) = {Bm, Bd, R1, R2}, "scale" (n, 4)}: shape (n, 5), status, field (n,), places (n, 2) the resident rows;
    mean, base, final the stacks (M, F, F, bands), base None for a set that keeps none (Bd NaN).  An ineligible row gets
    four NaN; a stamp wholly outside its field four zeros (Bd NaN without base)."""
    mean = np.asarray(mean, dtype=np.float64)
    final = np.asarray(final, dtype=np.float64)
    base = None if base is None else np.asarray(base, dtype=np.float64)
    n, F = len(status), mean.shape[1]
    out = dict(sums=np.full((n, 4), np.nan), scale=np.full((n, 4), np.nan))
    for i in range(n):
        if not bo.eligible(shape[i], status[i]):
            continue
        pr, pc, f = int(places[i][0]), int(places[i][1]), int(field[i])
        ra, rb = max(0, -pr), min(cs, F - pr)
        ca, cb = max(0, -pc), min(cs, F - pc)
        out["sums"][i], out["scale"][i] = 0.0, 0.0
        if rb > ra and cb > ca:
            g = bo.weights(cs, shape[i])[ra:rb, ca:cb]
            win = (f, slice(pr + ra, pr + rb), slice(pc + ca, pc + cb), band)
            x = final[win]
            terms = [mean[win], None if base is None else base[win], x, x * x]       # (the square rounded on its own)
            for k, t in enumerate(terms):
                if t is not None:
                    out["sums"][i, k] = total(g * t)
                    out["scale"][i, k] = total(g * np.abs(t))
        if base is None:
            out["sums"][i, 1] = out["scale"][i, 1] = np.nan
    return out
