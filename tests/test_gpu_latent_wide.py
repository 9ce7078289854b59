"""latent_dim above 64 (model.py:164 takes any value): the workgroup-per-stamp sampler kernels (sampler_wide_fwd_kernel,
sampler_wide_bwd_kernel) and the bf16 engine's mid backward (bt_mid_wide_bwd_kernel), against the fp64 oracle at the
tolerances of tests/test_gpu_parity.py::_run_parity and tests/test_gpu_bf16.py::_run, and through the public API."""
import numpy as np
import pytest

from oracle import vae_oracle as vo
from tests.test_gpu_parity import _run_parity

pytestmark = pytest.mark.gpu


def _toy(d, filters=(8, 16)):
    return vo.Arch(input_shape=(13, 13, 4), latent_dim=d, filters=filters, kernels=(3, 3))


def _wide_parity(arch, B, seed, train_decoder=True):
    """_run_parity's bounds (outputs 2e-4 * max, ELBO 1e-4 relative, gradients 1e-3 * max, 2e-3 for the BatchNorm pair)
    against the float64 oracle evaluated at the engine's own PReLU gate states (tests/test_gpu_parity.py::
    _gate_matched_gradients), except on the encoder tensors upstream of the encoder Dense's data gradient: 2.5e-3.  That
    product sums params_size terms per input (4752 at d = 96, 2144 at most below 65) in float32, and the conv-bias and
    PReLU-slope gradients behind it are small sums of it over 5 - 9 stamps with heavy cancellation.  Measured at d = 96 /
    100 on the MI355X: enc/prelu_flat/alpha 1.90e-3, enc/conv3/bias 1.31e-3, enc/conv1/bias 1.16e-3, enc/conv2/bias
    1.06e-3, identical with and without the gate matching (no gate flips); every tensor downstream of it, the encoder Dense
    and the sampler side included, within 1e-3."""
    from tests.test_gpu_parity import _case, _engine, _gate_matched_gradients, _grad_tol, _relmax

    p, x, y, eps = _case(arch, B, seed)
    eng = _engine(arch, max_batch=B)
    eng.set_params(p)
    eng.set_trainable(True, train_decoder)
    eng.optimizer_reset(1e-4)
    eng.upload(0, x, y)
    eng.keep_outputs(True)
    out = eng.grad_step(0, first=0, B=B, eps=eps)
    x64, y64, e64 = x.astype(np.float64), y.astype(np.float64), eps.astype(np.float64)
    c = vo.forward(arch, p, x64, e64, training=True)
    ref = vo.losses(arch, c, y64)
    d = arch.latent_dim
    for k, shape in (("t", (B, arch.params_size)), ("z", (B, d)), ("kl", (B,))):
        assert _relmax(eng.activation(k, shape), c[k]) <= 2e-4, k
    for k in ("loss", "nll_mean", "kl_reg", "mse"):
        assert abs(out[k] - ref[k]) <= 1e-4 * abs(ref[k]) + 1e-12, (k, out[k], ref[k])
    gm, _ = _gate_matched_gradients(eng, arch, p, x, y, eps, B, train_decoder)
    def tol(n):
        upstream = n.startswith("enc/") and not n.startswith("enc/dense/")
        return 2.5e-3 if upstream else _grad_tol(n)

    bad = [(n, _relmax(eng.get_grad(n), gm[n])) for n in gm if _relmax(eng.get_grad(n), gm[n]) > tol(n)]
    assert not bad, bad
    eng.close()


@pytest.mark.parametrize("latent", [65, 96, 100, 127, 128, 256])
def test_wide_latent_toy_arch(latent):
    # params_size = d + d (d + 1) / 2 is a multiple of 4 for none / some of these; 127 and 256 put rows of L across the
    # forward / reversed halves of fill_triangular and 256 gives every wave rows longer than one wavefront
    arch = _toy(latent)
    _wide_parity(arch, B=5, seed=240 + latent)
    _wide_parity(arch, B=9, seed=250 + latent, train_decoder=False)


def test_latent_dim_128_on_the_reference_architecture():
    from debvader_amd.data import synthetic_stamps

    arch = vo.Arch(latent_dim=128)
    x, y = synthetic_stamps(8, seed=21)
    _run_parity(arch, B=8, seed=66, data=(x, y), f32_floor=True)


@pytest.mark.parametrize("latent", [65, 128, 256])
def test_wide_latent_toy_arch_bf16(latent):
    # (filters 16 / 32: the dense layers of this toy net run unfused, the sampler backward is its own launch)
    from tests.test_gpu_bf16 import _run

    # (bound 1e-2 on the gradients against the bf16-rounding oracle instead of 5e-3: dec/prelu_in/alpha, d sums of five
    # stamps each, landed at 5.5e-3 at d = 65)
    _run(_toy(latent, (16, 32)), B=5, seed=260 + latent, tol_grad_b=1e-2, check_fp64_grads=False)


def test_latent_dim_128_on_the_reference_architecture_bf16():
    # the dense trunk on the matrix cores: the encoder Dense's K-split slabs finished by the wide sampler, the mid backward
    # in its wide form
    from debvader_amd.data import synthetic_stamps
    from tests.test_gpu_bf16 import _run

    x, y = synthetic_stamps(8, seed=22)
    # (gradients against the bf16-rounding oracle with the bounds of tests/test_gpu_bf16.py's few-stamp reference-architecture
    # case; against float64 only the outputs and the ELBO, as for the toy nets: at 8 stamps the format's own cost on
    # dec/dense0/kernel is a cosine of 0.62 to the float64 gradient where the engine matches the bf16 oracle)
    _run(vo.Arch(latent_dim=128), B=8, seed=67, data=(x, y), tol_grad_b=0.4, check_fp64_grads=False)


def test_wide_eps_matches_philox_and_extends_the_narrow_draw():
    """element (row, col) of the engine's draw uses Philox counter (row, col / 4, stream, 0) whatever latent_dim is: the
    first 64 columns of a d = 128 draw are, bit for bit, the draw of a d = 64 model with the same seed and rows."""
    from tests.test_gpu_parity import _case, _engine

    N = 7
    eps = {}
    for d in (64, 128):
        arch = _toy(d)
        p, x, _, _ = _case(arch, N, seed=31)
        eng = _engine(arch, max_batch=8)
        eng.set_params(p)
        eng.infer(x, seed=1234, want=("z", "mu"))
        eps[d] = eng.activation("eps", (N, d))
        eng.close()
    np.testing.assert_allclose(eps[128], vo.philox_normal(1234, 0, N, 128), rtol=0, atol=2e-5)
    np.testing.assert_array_equal(eps[128][:, :64], eps[64])


def test_wide_latent_max_batch_whose_t_rows_reach_two_to_the_31_is_refused():
    from debvader_amd import engine as E
    from debvader_amd._lib import DvError

    arch = _toy(256)                                   # 33 152 floats of t per stamp: more than any activation of this net
    tw = 256 + 256 * 257 // 2
    cfg = E.make_config(arch.input_shape, 256, tuple(arch.filters), tuple(arch.kernels), max_batch=(1 << 31) // tw + 1)
    with pytest.raises(DvError, match="largest activation reaches 2\\^31"):
        E.Engine(cfg)


def test_wide_latent_infer_mc_against_the_oracle():
    """tests/test_gpu_api.py::test_epistemic_monte_carlo_against_the_oracle_sample_by_sample at d = 100: the seed of
    sample s is seed + s, max_batch 16 < N * n (several decode passes)."""
    from debvader_amd import engine as E

    arch = _toy(100)
    p = vo.init_params(arch, seed=3, perturb=0.05)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    N, n, seed = 5, 12, 4321
    x = np.random.default_rng(19).normal(0, 0.4, size=(N, 13, 13, 4)).astype(np.float32)
    eng = E.Engine(E.make_config(arch.input_shape, arch.latent_dim, tuple(arch.filters), tuple(arch.kernels), max_batch=16))
    eng.set_params(p)
    t = vo.encoder_forward(arch, p, x.astype(np.float64), training=False)
    locs = []
    for s_ in range(n):
        eps = vo.philox_normal(seed + s_, 0, N, arch.latent_dim).astype(np.float64)
        z = vo.sampler_forward(arch, t, eps)[3]
        locs.append(vo.decoder_forward(arch, p, z)[0])
    locs = np.stack(locs)
    mean, std = eng.infer_mc(x, nsamples=n, seed=seed)
    ref_mean, ref_std = locs.mean(0), locs.std(0)
    assert np.abs(mean - ref_mean).max() <= 2e-4 * np.abs(ref_mean).max() + 1e-7
    assert np.abs(std - ref_std).max() <= 2e-4 * max(np.abs(ref_std).max(), np.abs(ref_mean).max()) + 1e-7
    eng.close()


def test_wide_latent_through_the_api_sub_models():
    from debvader_amd.data import synthetic_stamps
    from debvader_amd.model import model

    d = 100
    tw = d + d * (d + 1) // 2
    arch = _toy(d)
    net, encoder, decoder, z = model.create_model_vae((13, 13, 4), d, [8, 16], [3, 3], max_batch=8, seed=4)
    eng = net._core.engine
    p = vo.init_params(arch, seed=12, perturb=0.05)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    eng.set_params(p)
    x, _ = synthetic_stamps(11, seed=23, size=13, nb=4)
    t = encoder(x).numpy()
    ref_t = vo.encoder_forward(arch, p, x.astype(np.float64), training=False)
    assert t.shape == (11, tw)
    np.testing.assert_allclose(t, ref_t, rtol=0, atol=2e-4 * np.abs(ref_t).max())
    q = z(x)
    np.testing.assert_array_equal(q.mean().numpy(), t[:, :d])
    L = vo.sampler_forward(arch, ref_t, np.zeros((11, d)))[1]
    np.testing.assert_allclose(q.stddev().numpy(), np.sqrt((L ** 2).sum(-1)), rtol=2e-4)
    zz = np.random.default_rng(6).normal(size=(11, d)).astype(np.float32)
    loc, _ = vo.decoder_forward(arch, p, zz.astype(np.float64))
    np.testing.assert_allclose(decoder(zz).mean().numpy(), loc, rtol=0, atol=2e-4 * np.abs(loc).max())
    eng.close()


@pytest.mark.parametrize("fmt", ["ckpt", "npz"])
def test_wide_latent_weights_round_trip_bit_exact(tmp_path, fmt):
    from debvader_amd.data import synthetic_stamps
    from debvader_amd.model import model

    d = 128
    net, _, _, _ = model.create_model_vae((13, 13, 4), d, [8, 16], [3, 3], max_batch=8, seed=5)
    net.compile(optimizer=model.Adam(learning_rate=1e-3))
    eng = net._core.engine
    x, y = synthetic_stamps(8, seed=24, size=13, nb=4)
    eng.upload(0, x, y)
    eng.train_step(0, first=0, B=8, seed=9)                # (Adam slots non-zero)
    path = str(tmp_path / "w" / ("weights.npz" if fmt == "npz" else "weights.ckpt"))
    net.save_weights(path)
    net2, _, _, _ = model.create_model_vae((13, 13, 4), d, [8, 16], [3, 3], max_batch=8, seed=6)
    net2.compile(optimizer=model.Adam(learning_rate=1e-3))
    net2.load_weights(path)
    e2 = net2._core.engine
    for i, (name, shape, tr) in enumerate(eng.specs):
        np.testing.assert_array_equal(e2.get_param(i), eng.get_param(i), err_msg=name)
        if tr:
            np.testing.assert_array_equal(e2.get_slot(i, 0), eng.get_slot(i, 0), err_msg=name)
            np.testing.assert_array_equal(e2.get_slot(i, 1), eng.get_slot(i, 1), err_msg=name)
    assert dict((n, s) for n, s, _ in eng.specs)["enc/dense/kernel"] == (256, d + d * (d + 1) // 2)
    eng.close()
    e2.close()
