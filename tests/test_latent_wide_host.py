"""latent_dim above 64 (model.py:164 takes any value, params_size(d) = d + d (d + 1) / 2): the host side of the architecture
queries, which need no GPU.  What bounds latent_dim is the 32-bit element offsets of the kernels that address one
parameter tensor: the encoder Dense kernel [flat][params_size] must stay below 2^31 elements."""
import ctypes as C

import numpy as np
import pytest

from debvader_amd import engine as E
from debvader_amd._lib import DvError, check, lib
from oracle import vae_oracle as vo


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("d", [65, 96, 100, 128, 256, 512])
def test_wide_latent_specs_match_the_oracle(d, dtype):
    cfg = E.make_config(latent_dim=d, dtype=dtype)
    specs = E.arch_specs(cfg)
    assert specs == vo.Arch((59, 59, 6), d).param_specs()
    shapes = {n: s for n, s, _ in specs}
    tw = d + d * (d + 1) // 2
    assert shapes["enc/dense/kernel"] == (4096, tw) and shapes["dec/dense0/kernel"] == (d, 560)
    c = E.arch_counts(cfg)
    assert c["tensors"] == len(specs) == 64
    n_enc = sum(int(np.prod(s)) for n, s, _ in specs if n.startswith("enc/"))
    n_dec = sum(int(np.prod(s)) for n, s, _ in specs if n.startswith("dec/"))
    assert (c["encoder"], c["decoder"]) == (n_enc, n_dec)
    assert c["trainable"] == sum(int(np.prod(s)) for _, s, tr in specs if tr)
    # the gradient buckets still tile the trainable buffer and every tensor sits 16-byte aligned inside its class
    out = (C.c_int64 * 4)()
    check(lib.dv_arch_buckets(C.byref(cfg), out))
    split, n_enc_buf, n_train, n_total = list(out)
    assert 0 < split < n_enc_buf < n_train <= n_total and split % 4 == 0
    for i, (name, shape, trainable) in enumerate(specs):
        off, cnt = C.c_int64(), C.c_int64()
        check(lib.dv_arch_offset(C.byref(cfg), i, C.byref(off), C.byref(cnt)))
        assert cnt.value == int(np.prod(shape)) and off.value % 4 == 0
        if not trainable:
            assert off.value >= n_train
        elif name.startswith("dec/"):
            assert n_enc_buf <= off.value and off.value + cnt.value <= n_train
        else:
            assert off.value + cnt.value <= n_enc_buf
    enc, dec = E.arch_macs(cfg)
    enc32, dec32 = E.arch_macs(E.make_config(dtype=dtype))
    assert enc - enc32 == 4096 * (tw - 560) and dec - dec32 == (d - 32) * 560


@pytest.mark.parametrize("d", [65, 128])
def test_wide_latent_on_the_toy_architecture(d):
    cfg = E.make_config((13, 13, 4), d, (8, 16), (3, 3))
    assert E.arch_specs(cfg) == vo.Arch((13, 13, 4), d, (8, 16), (3, 3)).param_specs()


@pytest.mark.parametrize("dtype", [0, 1])
def test_latent_whose_dense_kernel_reaches_two_to_the_31_is_refused(dtype):
    # 4096 x 525 824 elements at d = 1024 on the reference architecture
    with pytest.raises(DvError, match="2\\^31 elements"):
        E.arch_counts(E.make_config(latent_dim=1024, dtype=dtype))
    # ... whatever the stamp size: a huge latent_dim must not overflow the size arithmetic
    with pytest.raises(DvError, match="2\\^31 elements"):
        E.arch_counts(E.make_config((13, 13, 4), 100_000, (8, 16), (3, 3)))
    big = E.make_config((13, 13, 4), 2048, (8, 16), (3, 3), dtype=dtype)       # 256 x 2 100 224: accepted
    assert E.arch_specs(big) == vo.Arch((13, 13, 4), 2048, (8, 16), (3, 3)).param_specs()
