"""Generates tests/golden/posfit.npz: the reference's own position fit on real and synthetic cases (run once in the build
container, where the reference and its sample data are; the GPU tests read only the .npz).

The reference's deblend_cutout/optimization.py is imported by file path and its position_optimization is called as
field_deblender.py:337-352 calls it: field (F, F, bands), the mean image padded to (F, F, bands), the distance to the
centre.  Only the r band (index 2) enters the fit, so only the r band is stored; the tests rebuild 3-band inputs with
zero g and i bands.

Cases (every one an integer distance unless stated):
  real       the DC2 field of the reference's sample data (data/dc2_imgs/field/field_img.npy) and stamps of
             galaxies_from_field.npy, each placed 1-2 px (integer) away from where its galaxy sits in the field, so the
             optimum is not the starting point; a galaxy whose default least_squares result is more than 2.5e-3 px from
             the same run to tight tolerances (a flat objective) is left out
  synthetic  a small noisy field of Gaussian galaxies: a fractional distance, a stamp within 20 px (the recursion
             margin) of the field edge, and a galaxy 4.5 px away from its distance so that the bound is active
Expected: the reference's (shift_x, shift_y) and J(shift) = mean((field_r - shift(shift(pad_r, d), s))^2).

Usage:  python tests/golden/make_posfit_golden.py
"""
import importlib.util
import os

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/debvader"


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pad(stamp_r, F):
    cs = stamp_r.shape[0]
    po = int((F - cs) / 2)
    out = np.zeros((F, F))
    out[po:po + cs, po:po + cs] = stamp_r
    return out


def objective(field_r, stamp_r, d, s):
    net = scipy.ndimage.shift(_pad(stamp_r, field_r.shape[0]), shift=(d[0], d[1]))
    return np.square(field_r - scipy.ndimage.shift(net, shift=(s[0], s[1]))).mean()


def _three_bands(a):
    out = np.zeros(a.shape + (3,))
    out[..., 2] = a
    return out


def _fit(opt, field_r, stamp_r, d):
    F = field_r.shape[0]
    sx, sy = opt.position_optimization(_three_bands(field_r), _three_bands(_pad(stamp_r, F)), d)
    return [sx, sy], objective(field_r, stamp_r, d, (sx, sy))


def _settled(opt, field_r, stamp_r, d, s):
    """True when the reference's default least_squares result lies within 2.5e-3 px (half the tests' tolerance) of the
    same least_squares run to tight tolerances: on a flat objective (a faint galaxy) the default tolerances stop it short
    of the optimum, and such a result pins nothing."""
    import scipy.optimize

    net = scipy.ndimage.shift(_pad(stamp_r, field_r.shape[0]), shift=(d[0], d[1]))
    fun = lambda x: np.square(field_r - scipy.ndimage.shift(net, shift=(x[0], x[1]))).mean()  # noqa: E731
    tight = scipy.optimize.least_squares(fun, (0.0, 0.0), bounds=(-3, 3), ftol=1e-15, xtol=1e-15, gtol=1e-15).x
    gap = float(np.abs(tight - np.asarray(s)).max())
    print(f"   default vs tight least_squares: {gap:.2e} px")
    return gap <= 2.5e-3


def _gauss(cs, sig, amp, e=0.0):
    y, x = np.mgrid[:cs, :cs] - (cs - 1) / 2.0
    return amp * np.exp(-0.5 * ((x / sig) ** 2 + (y / (sig * (1 + e))) ** 2))


def main():
    opt = _load(os.path.join(REF, "deblend_cutout/optimization.py"), "ref_optimization")
    field = np.load(os.path.join(REF, "data/dc2_imgs/field/field_img.npy"))[0, :, :, 2].astype(np.float64)
    gals = np.load(os.path.join(REF, "data/dc2_imgs/field/galaxies_from_field.npy"))[:, :, :, 2].astype(np.float64)
    F, cs = field.shape[0], gals.shape[1]
    po = int((F - cs) / 2)
    # where each galaxy sits: the integer distance whose placed stamp best matches the field
    rng = np.random.default_rng(7)
    real_d, real_s, real_j, real_stamp = [], [], [], []
    for g in gals:
        best, where = np.inf, None
        for dr in range(-po, po + 1):
            for dc in range(-po, po + 1):
                err = np.square(field[po + dr:po + dr + cs, po + dc:po + dc + cs] - g).sum()
                if err < best:
                    best, where = err, (dr, dc)
        off = rng.integers(1, 3, size=2) * rng.choice([-1, 1], size=2)
        d = [float(where[0] + off[0]), float(where[1] + off[1])]
        s, j = _fit(opt, field, g, d)
        if not _settled(opt, field, g, d, s):
            print("real", where, d, s, "left out: least_squares stops short of the optimum")
            continue
        real_d.append(d); real_s.append(s); real_j.append(j); real_stamp.append(g)
        print("real", where, d, s, j)

    # synthetic: F = 81, cs = 21 (po = 30)
    Fs, css = 81, 21
    sfield = rng.normal(0, 0.05, size=(Fs, Fs))
    pos = {"frac": (2.4, -3.7), "edge": (-27.0, 26.0), "bound": (12.0, -14.0)}
    true_shift = {"frac": (0.6, 1.3), "edge": (-1.2, 0.7), "bound": (4.5, -1.0)}
    shapes = {"frac": _gauss(css, 2.5, 3.0, 0.2), "edge": _gauss(css, 2.0, 4.0, -0.1), "bound": _gauss(css, 3.0, 2.0, 0.3)}
    for k in pos:
        sfield += scipy.ndimage.shift(_pad(shapes[k], Fs), shift=(pos[k][0] + true_shift[k][0], pos[k][1] + true_shift[k][1]))
    syn_d, syn_s, syn_j, syn_stamp = [], [], [], []
    for k in pos:
        s, j = _fit(opt, sfield, shapes[k], pos[k])
        assert _settled(opt, sfield, shapes[k], pos[k], s), k
        syn_d.append(list(pos[k])); syn_s.append(s); syn_j.append(j); syn_stamp.append(shapes[k])
        print("synthetic", k, pos[k], s, j)

    np.savez_compressed(os.path.join(HERE, "posfit.npz"),
                        real_field_r=field, real_stamps_r=np.array(real_stamp), real_dist=np.array(real_d),
                        real_shift=np.array(real_s), real_objective=np.array(real_j),
                        syn_field_r=sfield, syn_stamps_r=np.array(syn_stamp), syn_dist=np.array(syn_d),
                        syn_shift=np.array(syn_s), syn_objective=np.array(syn_j), syn_names=np.array(list(pos)))
    print("wrote", os.path.getsize(os.path.join(HERE, "posfit.npz")), "bytes")


if __name__ == "__main__":
    main()
