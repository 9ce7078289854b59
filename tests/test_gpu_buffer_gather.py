"""Range-checked buffer gathers of the gather-GEMM kernels (gconv2.hip, gconv_s2.hip) against the select form they replace.

Both forms feed the same MFMAs the same operands in the same order, so every comparison here is of BIT PATTERNS: the
count of differing output words must be 0, not small.  The gather cross-check (dv_debug_gconv_check with bit 8 of its
epilogue argument set; the tile code + 1 travels in bits 16-23) places X and W inside larger allocations
between two 64 KiB bands of NaN and hands the kernels descriptors that cover the tensors alone: a load that strays past a
tensor reads a NaN out of the same allocation (a wrong value, never a fault), a lane that should have read zeros and did
not shows as a differing word.

The uniform per-step offsets (tap, channel chunk, weight tap) are part of the per-lane offset operand in both kernels; the
scalar offset operand of the loads is 0 everywhere, so there is no case for it here.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATHER_CHECK = 0x100        # bit 8 of dv_debug_gconv_check's epilogue argument: the gather cross-check, three floats out
SELECT_GATHERS = 2          # bit 1 of dv_debug_general_kernels: the select form of the gconv2 / gconv_s2 gathers


def _run(cases, winograd=1):
    """cases: (NB, Hs, Cs, Ht, Ct, stride, pad_before, dgrad_form, nmajor, epi, tile)"""
    from debvader_amd import engine as E
    from debvader_amd._lib import check
    from tests import debug_lib

    out = (C.c_float * 3)()
    with debug_lib.debug_build() as lib:
        ctx = E.default_context()
        check(lib.dv_debug_winograd(winograd))
        try:
            for c in cases:
                out[0] = out[1] = out[2] = -1.0
                *shape, epi, tile = c
                check(lib.dv_debug_gconv_check(ctx._h, *shape, GATHER_CHECK | epi | ((tile + 1) << 16), out))
                assert out[2] > 0.1, (c, "nothing was computed", out[2])
                assert out[0] == 0, (c, f"{int(out[0])} output words differ between the select and the buffer path")
                assert out[1] == 0, (c, f"{int(out[1])} NaNs in the buffer path's outputs")
        finally:
            check(lib.dv_debug_winograd(1))


def test_stride2_forward_form_gconv2():
    """Conv2D stride 2 (model.py:33-70): odd inputs whose last output row / column reaches past the image (59 -> 30,
    15 -> 8, 9 -> 5, SAME padding: one pixel in front), 32 -> 32 / 36 / 64 channels (36 is ragged against every column
    tile), both weight layouts, one and three stamps (M below and above one tile)."""
    cases = []
    for NB in (1, 3):
        for (hs, ht) in ((59, 30), (15, 8), (9, 5)):
            for ct in (32, 36, 64):
                cases.append((NB, hs, 32, ht, ct, 2, 1, 0, 0, 2, -1))
            cases.append((NB, hs, 32, ht, 36, 2, 1, 0, 1, 0, -1))
    _run(cases)


def test_every_gconv2_tile_form():
    """The eight tile forms are separate instantiations: each on a shape with partial row tiles and ragged columns."""
    cases = []
    for tile in range(8):
        for nmajor in (0, 1):
            cases.append((3, 15, 32, 8, 36, 2, 1, 0, nmajor, 2, tile))
            cases.append((1, 9, 64, 5, 132, 2, 1, 0, nmajor, 1, tile))
    _run(cases)


def test_stride2_transposed_form_gconv_s2():
    """Conv2DTranspose stride 2 / the data gradient of a stride-2 Conv2D (model.py:86-110): 4 -> 8 (even, no pad),
    8 -> 15 and 30 -> 59 (odd outputs: the class-validity bits drop the last row / column of three classes), 32 / 64 ->
    32 / 36 channels; the half-height tile the dispatcher takes below 512 workgroups (automatic at these sizes) and the
    128 x 32 tile of the larger rule (tile code 1), the latter also at 16 stamps of 30 -> 59.  NB = 1 at 4 -> 8 has 16
    base pixels: most rows of the tile lie beyond M."""
    cases = []
    for NB in (1, 3):
        for (hs, ht, pb) in ((4, 8, 0), (8, 15, 1), (30, 59, 1)):
            for cs in (32, 64):
                for ct in (32, 36):
                    for tile in (-1, 1):
                        cases.append((NB, hs, cs, ht, ct, 2, pb, 1, 1, 2, tile))
            cases.append((NB, hs, 32, ht, 36, 2, pb, 1, 1, 0, -1))
    cases.append((16, 30, 32, 59, 32, 2, 1, 1, 1, 2, 1))
    for tile in (0, 2, 3):                               # the other tile forms of the family
        cases.append((3, 8, 64, 15, 36, 2, 1, 1, 1, 2, tile))
    _run(cases)


def test_other_gconv2_modes():
    """Dense 1 x 1 (one tap, Hs = Ht = 1; with 560 inputs the ragged-K form), a stride-1 3 x 3 layer with the Winograd
    kernel switched off (forward and data-gradient form), the parity-class data gradient of gconv2 (k-major weights
    keep it away from gconv_s2), and the forms with 8 and 16 input channels (several taps per K chunk)."""
    cases = []
    for NB in (1, 3):
        for nmajor in (0, 1):
            cases.append((NB, 1, 64, 1, 36, 1, 0, 0, nmajor, 1, -1))
            cases.append((NB, 1, 560, 1, 64, 1, 0, 0, nmajor, 2, -1))
        cases.append((NB, 30, 32, 30, 64, 1, 1, 0, 0, 2, -1))
        cases.append((NB, 30, 32, 30, 64, 1, 1, 1, 1, 2, -1))
        cases.append((NB, 8, 32, 15, 36, 2, 1, 1, 0, 2, -1))
        cases.append((NB, 5, 8, 5, 32, 1, 1, 0, 0, 2, -1))
        cases.append((NB, 5, 16, 5, 32, 1, 1, 0, 0, 2, -1))
        cases.append((NB, 9, 16, 5, 16, 2, 1, 0, 0, 1, -1))
        cases.append((NB, 5, 16, 9, 32, 2, 1, 1, 1, 2, -1))
    _run(cases, winograd=0)


@pytest.mark.parametrize("filters", [(8, 16), (32, 64)])
def test_whole_step_is_bit_identical(filters):
    """Three train steps of the 13 x 13 toy net of tests/test_gpu_parity.py at 5 stamps (and of the same net with 32 / 64
    filters, whose stride-2 layers reach gconv_s2) with the select gathers and with the buffer gathers: every parameter
    and every scalar the steps return are bit-equal."""
    from debvader_amd import engine as E
    from debvader_amd._lib import check
    from oracle import vae_oracle as vo
    from tests import debug_lib
    from tests.test_gpu_parity import _case

    arch = vo.Arch(input_shape=(13, 13, 4), latent_dim=8, filters=filters, kernels=(3, 3))
    B = 5
    p, x, y, eps = _case(arch, B, seed=11)
    runs = []
    with debug_lib.debug_build() as lib:
        try:
            for select in (SELECT_GATHERS, 0):
                check(lib.dv_debug_general_kernels(select))
                cfg = E.make_config(arch.input_shape, arch.latent_dim, tuple(arch.filters), tuple(arch.kernels), max_batch=B)
                eng = E.Engine(cfg)
                eng.set_params(p)
                eng.upload(0, x, y)
                scalars = [eng.train_step(0, first=0, B=B, eps=eps) for _ in range(3)]
                runs.append((scalars, {k: np.array(v, copy=True) for k, v in eng.get_params().items()}))
        finally:
            check(lib.dv_debug_general_kernels(0))
    (s0, p0), (s1, p1) = runs
    for a, b in zip(s0, s1):
        assert a.keys() == b.keys()
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (k, a[k], b[k])
    assert p0.keys() == p1.keys() and len(p0) > 0
    for k in p0:
        assert p0[k].tobytes() == p1[k].tobytes(), k
    assert np.isfinite(s1[-1]["loss"])
