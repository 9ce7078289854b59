"""numpy float64 restatement of the blendedness sums (csrc/blend.hip), for the tests.  Per galaxy, over
the stamp pixels that lie inside the field, in plain raster order: W = sum g, A = sum g P, Bm = sum g T, Bd = sum g D with g
the Gaussian of the galaxy's adaptive moments; also sum g |x| for the three value sums, the scale of their rounding error."""
import numpy as np


def eligible(shape, status):
    shape = np.asarray(shape, dtype=np.float64)
    if int(status) not in (0, 2) or not np.isfinite(shape).all():
        return False
    with np.errstate(all="ignore"):
        det = shape[2] * shape[4] - shape[3] * shape[3]
    return bool(np.isfinite(det) and det > 1e-6)


def weights(cs, shape):
    """g [cs][cs] of an eligible row, the operations in the order of the definition"""
    r0, c0, Mrr, Mrc, Mcc = (float(v) for v in shape)
    det = Mrr * Mcc - Mrc * Mrc
    qa, qb, qc = -0.5 * Mcc / det, Mrc / det, -0.5 * Mrr / det
    dr = np.arange(cs, dtype=np.float64)[:, None] - r0
    dc = np.arange(cs, dtype=np.float64)[None, :] - c0
    return np.exp(qa * dr * dr + qb * dr * dc + qc * dc * dc)


def raster_sum(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    return float(np.add.accumulate(x)[-1]) if x.size else 0.0      # (accumulate adds strictly in order)


def blend(stamps, shape, status, places, model_fields, data_fields=None, field_ptr=None, band=2, total=raster_sum):
    """{"blend" (N, 4), "npix" (N,), "abs" (N, 3): sum g |x| for A, Bm, Bd}; `total` sums a raster-ordered array"""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs = stamps.shape[0], stamps.shape[1]
    model = np.asarray(model_fields, dtype=np.float64)
    data = None if data_fields is None else np.asarray(data_fields, dtype=np.float64)
    M, F = model.shape[0], model.shape[1]
    fp = np.array([0, n]) if field_ptr is None else np.asarray(field_ptr)
    field = np.repeat(np.arange(M), np.diff(fp))
    out = dict(blend=np.full((n, 4), np.nan), npix=np.full(n, -1, np.int32), abs=np.full((n, 3), np.nan))
    for i in range(n):
        if not eligible(shape[i], status[i]):
            continue
        pr, pc = int(places[i][0]), int(places[i][1])
        ra, rb = max(0, -pr), min(cs, F - pr)
        ca, cb = max(0, -pc), min(cs, F - pc)
        if rb <= ra or cb <= ca:
            out["blend"][i], out["npix"][i], out["abs"][i] = 0.0, 0, 0.0
            continue
        g = weights(cs, shape[i])[ra:rb, ca:cb]
        P = stamps[i, ra:rb, ca:cb, band].astype(np.float64)
        T = model[field[i], pr + ra:pr + rb, pc + ca:pc + cb, band]
        vals = [P, T] + ([data[field[i], pr + ra:pr + rb, pc + ca:pc + cb, band]] if data is not None else [])
        out["npix"][i] = g.size
        out["blend"][i, 0] = total(g)
        for k, x in enumerate(vals):
            out["blend"][i, 1 + k] = total(g * x)
            out["abs"][i, k] = total(g * np.abs(x))
    return out


def composite(stamps, places, field_ptr, M, F):
    """T: the sum of every field's stamps at their placements, in object order, off-field parts dropped"""
    stamps = np.asarray(stamps, dtype=np.float32)
    n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
    out = np.zeros((M, F, F, nb))
    field = np.repeat(np.arange(M), np.diff(np.asarray(field_ptr)))
    for i in range(n):
        pr, pc = int(places[i][0]), int(places[i][1])
        ra, rb, ca, cb = max(0, -pr), min(cs, F - pr), max(0, -pc), min(cs, F - pc)
        if rb > ra and cb > ca:
            out[field[i], pr + ra:pr + rb, pc + ca:pc + cb] += stamps[i, ra:rb, ca:cb].astype(np.float64)
    return out


def ratios(blend, npix):
    """(blendedness, blendedness_data) as the Python layer derives them"""
    blend, npix = np.asarray(blend, dtype=np.float64), np.asarray(npix)
    res = []
    with np.errstate(all="ignore"):
        for B in (blend[:, 2], blend[:, 3]):
            res.append(np.array([1.0 - a / b if k >= 0 and b > 0 else np.nan for a, b, k in zip(blend[:, 1], B, npix)]))
    return res
