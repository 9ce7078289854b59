"""GPU tests of the drop-in Python surface (create_model_vae / train_deblender / deblend) and of
size-independent properties at the BASELINE batch size (256 stamps of 59x59x6)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARCH = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])


def _data(n, seed):
    from debvader_amd.data import synthetic_stamps

    return synthetic_stamps(n, seed=seed)


def test_fit_history_and_deblend_like_the_training_notebook(tmp_path, capsys):
    from debvader_amd.deblend_cutout.deblender import deblend
    from debvader_amd.model import model
    from debvader_amd.training.metrics import vae_loss

    net, encoder, decoder, z = model.create_model_vae(**ARCH, max_batch=8)
    assert "in cropping" in capsys.readouterr().out            # model.py:142 prints it for 59-px stamps
    with pytest.raises(RuntimeError):
        net.fit(np.zeros((1, 59, 59, 6)), np.zeros((1, 59, 59, 6)))

    def kl_metric(y_true, y_pred):
        return sum(net.losses)

    net.compile(optimizer=model.Adam(learning_rate=1e-4), loss=vae_loss, metrics=["mse", kl_metric],
                experimental_run_tf_function=False)
    x, y = _data(12, 1)
    xv, yv = _data(5, 2)
    hist = net.fit(x, y, epochs=2, batch_size=5, verbose=0, shuffle=True, validation_data=(xv, yv),
                   validation_steps=1)
    assert sorted(hist.history) == ["kl_metric", "loss", "mse", "val_kl_metric", "val_loss", "val_mse"]
    assert all(len(v) == 2 and np.isfinite(v).all() for v in hist.history.values())
    assert net._core.engine.iterations == 2 * 3                 # 12 stamps / batch 5 -> 3 steps (last partial batch used)
    assert len(net.losses) == 2 and abs(sum(net.losses) - hist.history["val_kl_metric"][-1]) < 1e-6

    mean, dist = deblend(net, x[:3].astype(np.float64))
    assert mean.shape == (3, 59, 59, 6) and mean.dtype == np.float32
    assert dist.stddev().numpy().min() >= 1e-4 * (1 - 1e-6)
    assert dist.sample(4).shape == (4, 3, 59, 59, 6) and dist.log_prob(y[:3]).shape == (3, 59, 59, 6)
    # epistemic-uncertainty usage (field_deblender.py:303-313): repeated decodes of one stamp must vary
    rep, _ = deblend(net, np.repeat(x[:1], 16, axis=0))
    assert np.std(rep, axis=0).max() > 0
    # sub-models share the weights
    t = encoder(x[:2])
    assert t.numpy().shape == (2, 560)
    q = z(x[:2])
    np.testing.assert_allclose(q.mean().numpy(), t[:, :32], rtol=0, atol=0)
    assert q.stddev().numpy().shape == (2, 32) and (q.stddev().numpy() > 0).all()
    d = decoder(q.mean())
    assert d.mean().numpy().shape == (2, 59, 59, 6)
    # normalise=True: evident intent of deblender.py:14-22
    mn, _ = deblend(net, x[:2], normalise=True)
    assert np.isfinite(mn).all()

    # checkpoint round trip (ModelCheckpoint(save_weights_only=True) semantics)
    before = net.get_weights()
    net.save_weights(str(tmp_path / "w" / "weights_noisy_v4.ckpt"))
    net.fit(x, y, epochs=1, batch_size=6, verbose=0)
    assert any(np.abs(a - b).max() > 0 for a, b in zip(before, net.get_weights()))
    net.load_weights(model.latest_checkpoint(str(tmp_path / "w")))
    for a, b in zip(before, net.get_weights()):
        np.testing.assert_array_equal(a, b)


def test_train_deblender_two_stages_freezes_decoder(monkeypatch, tmp_path):
    from debvader_amd.model import model
    from debvader_amd.training import train

    monkeypatch.setattr(model, "weights_dir", lambda survey: str(tmp_path / str(survey)))
    x, y = _data(5, 3)
    xv, yv = _data(5, 4)
    captured = {}
    orig = train.train_network

    def spy(net, *a, **k):
        captured.setdefault("dec", []).append(net._core.engine.get_param("dec/convt3/kernel"))
        captured.setdefault("enc", []).append(net._core.engine.get_param("enc/conv3/kernel"))
        return orig(net, *a, **k)

    monkeypatch.setattr(train, "train_network", spy)
    hv, hd, net = train.train_deblender("dc2_test", None, 2, (x, y), (xv, yv), (x, y), (xv, yv), nb_of_bands=6,
                                        batch_size=5, with_callbacks=True, verbose=2)
    assert set(hv.history) == {"loss", "mse", "kl_metric", "val_loss", "val_mse", "val_kl_metric"}
    eng = net._core.engine
    dec_after, enc_after = eng.get_param("dec/convt3/kernel"), eng.get_param("enc/conv3/kernel")
    assert np.abs(captured["dec"][1] - captured["dec"][0]).max() > 0        # stage 1 trains the decoder
    np.testing.assert_array_equal(dec_after, captured["dec"][1])            # stage 2 leaves it untouched
    assert np.abs(enc_after - captured["enc"][1]).max() > 0                 # ... and trains the encoder
    assert eng.iterations == 2                                              # fresh Adam after re-compile (train.py:178)
    assert (tmp_path / "dc2_test" / "vae" / "val_loss" / "checkpoint").exists()
    with pytest.raises(ValueError):
        train.train_deblender("s", None, 1, (x[..., :5], y[..., :5]), (xv, yv), (x, y), (xv, yv), nb_of_bands=6)


def test_full_batch_determinism_and_permutation_invariance():
    """BASELINE configs[1] size (B=256): same inputs twice -> bit-identical update; permuting the stamps
    (and their eps) changes only the summation order."""
    from debvader_amd import engine as E

    B = 256
    x, y = _data(B, 7)
    eps = np.random.default_rng(1).normal(size=(B, 32)).astype(np.float32)
    res = []
    for perm in (np.arange(B), np.arange(B), np.random.default_rng(2).permutation(B)):
        eng = E.Engine(E.make_config(max_batch=B))
        eng.init(seed=5)
        eng.optimizer_reset(1e-4)
        eng.upload(0, x[perm], y[perm])
        out = eng.grad_step(0, first=0, B=B, eps=eps[perm])
        res.append((out, eng.get_grad("dec/convt5/kernel"), eng.get_grad("enc/conv0/kernel"),
                    eng.get_grad("enc/prelu2/alpha"), eng.get_grad("enc/dense/bias")))
        eng.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        np.testing.assert_array_equal(a, b)
    assert np.isfinite(res[0][0]["loss"])
    assert abs(res[0][0]["loss"] - res[2][0]["loss"]) <= 1e-5 * abs(res[0][0]["loss"])
    for a, b in zip(res[0][1:], res[2][1:]):
        assert np.abs(a - b).max() <= 1e-3 * np.abs(a).max()


def test_queued_train_steps_are_bit_reproducible_at_full_batch():
    """Six queued B=256 train steps (weight gradients on the aux stream, reductions and early Adam on two more
    streams) on fresh engines: every parameter must come out bit-identical - a race between the streams would not."""
    from debvader_amd import engine as E

    B = 256
    x, y = _data(2 * B, 11)
    res = []
    for _ in range(3):
        eng = E.Engine(E.make_config(max_batch=B))
        eng.init(seed=5)
        eng.optimizer_reset(1e-4)
        eng.upload(0, x, y)
        out = eng.train_steps(0, 0, B, 6, seed=10)
        res.append((out["loss"], [eng.get_param(n) for n, _, tr in eng.specs if tr]))
        eng.close()
    assert np.isfinite(res[0][0])
    for loss, params in res[1:]:
        assert loss == res[0][0]
        for a, b in zip(res[0][1], params):
            np.testing.assert_array_equal(a, b)


def test_train_steps_queue_matches_stepwise():
    from debvader_amd import engine as E

    x, y = _data(16, 9)
    outs = []
    for mode in ("queue", "step"):
        eng = E.Engine(E.make_config(max_batch=8))
        eng.init(seed=3)
        eng.optimizer_reset(1e-4)
        eng.upload(0, x, y)
        if mode == "queue":
            o = eng.train_steps(0, 0, 8, 3, seed=10)
        else:
            for k in range(3):
                o = eng.train_step(0, first=(k * 8) % 9, B=8, seed=10 + k)
        outs.append((o, eng.get_param("dec/head/kernel")))
        eng.close()
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_collective_code_path_with_one_rank_communicator():
    """DV_FORCE_COMM builds a 1-rank RCCL communicator so the multi-GPU code path (comm stream, events, in-place
    all-reduces of BN sums / loss sums / both gradient buckets) executes on this single-GPU box; it must not
    change a single bit of the update."""
    import os
    import subprocess
    import sys

    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from debvader_amd import engine as E
from debvader_amd.data import synthetic_stamps
from debvader_amd._lib import check
if "fuse" in sys.argv[1:]:          # the parked fused epilogue lives in the development build of the library
    from tests import debug_lib
    check(debug_lib.use_for_process().dv_debug_fuse_prelu_bwd(1))
x, y = synthetic_stamps(16, seed=3)
eng = E.Engine(E.make_config(max_batch=8))
eng.init(seed=4); eng.optimizer_reset(1e-4); eng.upload(0, x, y)
out = eng.train_steps(0, 0, 8, 3, seed=7)
w = eng.get_param("dec/convt5/kernel"); v = eng.get_param("enc/conv0/kernel")
print(repr(out["loss"]), float(np.abs(w).sum()), float(np.abs(v).sum()), float(eng.ctx.allreduce([1.5, 2.5]).sum()))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for force in ("", "1", "fuse"):
        env = dict(os.environ)
        env.pop("DV_FORCE_COMM", None)
        if force == "1":
            env["DV_FORCE_COMM"] = "1"
        # "fuse": the parked fused PReLU-backward epilogue (debvader_hip_debug.h): same math, different summation order
        r = subprocess.run([sys.executable, "-c", code % root] + (["fuse"] if force == "fuse" else []), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1], outs
    assert outs[0].endswith(" 4.0")
    a, b = [float(v) for v in outs[0].split()], [float(v) for v in outs[2].split()]
    assert all(abs(x - y) <= 1e-4 * abs(x) for x, y in zip(a, b)), (outs[0], outs[2])


def test_epistemic_monte_carlo_matches_the_reference_loop_statistically():
    """deblend_epistemic (encode once, decode n times, Welford on the GPU) versus the reference's recipe
    np.std(deblend(net, [stamp]*n)[0], axis=0) (field_deblender.py:303-313) run through the same engine."""
    from debvader_amd.deblend_cutout.deblender import deblend, deblend_epistemic
    from debvader_amd.model import model

    net, enc, dec, z = model.create_model_vae(**ARCH, max_batch=64)
    x, _ = _data(3, 11)
    n = 256
    mean, std = deblend_epistemic(net, x, n_samples=n)
    assert mean.shape == x.shape and std.shape == x.shape and np.isfinite(mean).all() and (std >= 0).all()
    ref_std = np.stack([np.std(deblend(net, np.repeat(x[i:i + 1], n, axis=0))[0], axis=0) for i in range(3)])
    ref_mean = np.stack([np.mean(deblend(net, np.repeat(x[i:i + 1], n, axis=0))[0], axis=0) for i in range(3)])
    big = ref_std > 0.1 * ref_std.max()
    assert big.sum() > 10
    # two independent Monte-Carlo estimates with n samples each: the std agrees within a few sigma/sqrt(2n)
    assert np.abs(std[big] / ref_std[big] - 1).mean() < 0.1
    assert np.abs(mean - ref_mean).max() <= 6 * (ref_std.max() / np.sqrt(n)) + 1e-6
    # with one sample the spread is zero and the mean is a single decode
    m1, s1 = deblend_epistemic(net, x, n_samples=1)
    assert np.abs(s1).max() == 0 and np.isfinite(m1).all()


def test_epistemic_monte_carlo_against_the_oracle_sample_by_sample():
    """dv_infer_mc draws the noise of (stamp i, sample s) from the engine's Philox stream (seed + s, row i); the oracle
    reproduces every draw with vo.philox_normal, decodes each sample and takes the mean and the ddof-0 standard deviation
    over the samples (the reference's np.std(deblend(net, [stamp]*n)[0], axis=0), field_deblender.py:303-313).
    Tolerance: 2e-4 * max per tensor.  With normalise=True the statistics are those of the DENORMALISED means."""
    from oracle import vae_oracle as vo
    from debvader_amd import engine as E

    arch = vo.Arch(input_shape=(13, 13, 4), latent_dim=8, filters=(8, 16), kernels=(3, 3))
    p = vo.init_params(arch, seed=3, perturb=0.05)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    rng = np.random.default_rng(17)
    N, n, seed = 5, 12, 1234
    x = rng.normal(0, 0.4, size=(N, 13, 13, 4)).astype(np.float32)
    # max_batch 16 < N * n: the decodes run in several passes of 3 samples each (16 // 5)
    eng = E.Engine(E.make_config(arch.input_shape, arch.latent_dim, tuple(arch.filters), tuple(arch.kernels), max_batch=16))
    eng.set_params(p)
    for normalise in (False, True):
        xin = np.tanh(np.arcsinh(x.astype(np.float64))) if normalise else x.astype(np.float64)
        t = vo.encoder_forward(arch, p, xin, training=False)
        locs = []
        for s_ in range(n):
            eps = vo.philox_normal(seed + s_, 0, N, arch.latent_dim).astype(np.float64)
            _, _, _, z, _ = vo.sampler_forward(arch, t, eps)
            loc, _ = vo.decoder_forward(arch, p, z)
            locs.append(np.sinh(np.arctanh(loc)) if normalise else loc)
        locs = np.stack(locs)
        eng.set_normalise(normalise)
        mean, std = eng.infer_mc(x, nsamples=n, seed=seed)
        eng.set_normalise(False)
        ref_mean, ref_std = locs.mean(0), locs.std(0)
        assert np.abs(mean - ref_mean).max() <= 2e-4 * np.abs(ref_mean).max() + 1e-7, normalise
        assert np.abs(std - ref_std).max() <= 2e-4 * max(np.abs(ref_std).max(), np.abs(ref_mean).max()) + 1e-7, normalise
    eng.close()


def test_pipelined_inference_matches_chunked_calls_bit_for_bit():
    """dv_infer stages long inputs through a pinned three-stage pipeline (engine.hip: infer_pipelined); short inputs
    take the plain path.  Same kernels, same per-stamp noise: the results must be identical, for float32 and for
    float64 input (the cast of deblender.py:18 then happens inside the library), ragged last chunk included."""
    from debvader_amd.model import model

    net, enc, dec, z = model.create_model_vae(**ARCH, max_batch=128)
    eng = net._core.engine
    N = 128 * 4 + 37
    x, _ = _data(64, 21)
    x = np.concatenate([x] * 9)[:N] * np.linspace(0.5, 1.5, N, dtype=np.float32)[:, None, None, None]
    eps = np.random.default_rng(5).normal(size=(N, 32)).astype(np.float32)
    want = ("loc", "scale", "mu", "zstd", "z")
    full = eng.infer(x, eps=eps, want=want)                       # N > 256: pipelined, chunks of 128
    parts = [eng.infer(x[o:o + 200], eps=eps[o:o + 200], want=want) for o in range(0, N, 200)]   # <= 256: plain path
    for k in want:
        np.testing.assert_array_equal(full[k], np.concatenate([p[k] for p in parts]), err_msg=k)
    full64 = eng.infer(x.astype(np.float64), eps=eps, want=want)  # dv_infer_f64
    for k in want:
        np.testing.assert_array_equal(full64[k], full[k], err_msg=k + " (float64 input)")
    # engine-generated noise: rows are numbered globally, so the chunking does not change the sample either
    a = eng.infer(x, seed=9, want=("loc", "z"))
    b = eng.infer(x, seed=9, want=("loc", "z"), out={"loc": np.empty_like(a["loc"])})
    np.testing.assert_array_equal(a["loc"], b["loc"])
    np.testing.assert_array_equal(a["z"][:200], eng.infer(x[:200], seed=9, want=("z",))["z"])


def test_normalise_runs_on_the_gpu_and_matches_the_reference_transforms():
    """deblend(normalise=True): tanh(arcsinh(x)) before the network and sinh(arctanh(.)) on the mean
    (normalize/normalize.py:3-7), both as GPU kernels.  Checked against the same forward pass fed with inputs
    normalised on the host by the reference-pinned functions (tests/golden/helpers.npz pins those)."""
    from debvader_amd.deblend_cutout.deblender import deblend
    from debvader_amd.model import model
    from debvader_amd.normalize.normalize import denormalize_non_linear, normalize_non_linear

    net, enc, dec, z = model.create_model_vae(**ARCH, max_batch=64)
    eng = net._core.engine
    x, _ = _data(6, 31)
    x = x * 3.0                                   # reach the non-linear part of the transform
    eps = np.random.default_rng(2).normal(size=(6, 32)).astype(np.float32)
    ref = eng.infer(normalize_non_linear(x.astype(np.float64)).astype(np.float32), eps=eps)
    eng.set_normalise(True)
    try:
        got = eng.infer(x, eps=eps)
    finally:
        eng.set_normalise(False)
    want_mean = denormalize_non_linear(np.clip(ref["loc"].astype(np.float64), -1 + 1e-7, 1 - 1e-7))
    np.testing.assert_allclose(got["loc"], want_mean, rtol=2e-5, atol=1e-6)     # float32 transforms on the device
    np.testing.assert_allclose(got["scale"], ref["scale"], rtol=2e-5, atol=1e-7)
    mean, dist = deblend(net, x, normalise=True)
    assert mean.shape == x.shape and np.isfinite(mean).all() and (dist.stddev().numpy() > 0).all()
    # the flag does not leak into later calls
    np.testing.assert_array_equal(eng.infer(x, eps=eps)["loc"], eng.infer(x, eps=eps)["loc"])
    assert np.abs(eng.infer(x, eps=eps)["loc"] - got["loc"]).max() > 0


def test_training_reduces_the_loss_on_a_small_set():
    """End-to-end sanity of forward + ELBO + backward + Adam through the drop-in API: a few epochs on 96 synthetic
    stamps must bring the ELBO down substantially (lr 1e-3 to make it quick) and keep everything finite."""
    from debvader_amd.model import model
    from debvader_amd.training.metrics import vae_loss

    x, y = _data(96, 41)
    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=32)
    net.compile(optimizer=model.Adam(learning_rate=1e-3), loss=vae_loss, metrics=["mse"])
    h = net.fit(x, y, epochs=6, batch_size=32, verbose=0, validation_data=(x[:32], y[:32]))
    loss = h.history["loss"]
    assert all(np.isfinite(v) for v in loss) and all(np.isfinite(v) for v in h.history["val_loss"])
    assert loss[-1] < 0.5 * loss[0], loss
    assert all(np.isfinite(v) for v in h.history["mse"])      # (mse compares with a SAMPLE of the output distribution)
    assert all(np.isfinite(w).all() for w in net.get_weights())


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_edge_cases_empty_and_ragged_inputs(dtype):
    """Empty inputs, a single stamp, a data set smaller than the batch, the largest batch the workspace takes and one
    more (which must be refused with a message, not crash) - on both engines."""
    from debvader_amd._lib import DvError
    from debvader_amd.deblend_cutout.deblender import deblend
    from debvader_amd.model import model
    from debvader_amd.training.metrics import vae_loss

    net, enc, dec, z = model.create_model_vae(**ARCH, max_batch=8, dtype=dtype)
    x, y = _data(11, 51)
    mean, dist = deblend(net, x[:0])
    assert mean.shape == (0, 59, 59, 6) and dist.stddev().numpy().shape == (0, 59, 59, 6)
    mean, _ = deblend(net, x[:1])
    assert mean.shape == (1, 59, 59, 6) and np.isfinite(mean).all()
    mean, _ = deblend(net, x)                      # 11 stamps through an 8-stamp workspace: two chunks
    assert mean.shape == x.shape and np.isfinite(mean).all()
    assert enc(x[:0]).numpy().shape == (0, 560)
    net.compile(optimizer=model.Adam(learning_rate=1e-4), loss=vae_loss, metrics=["mse"])
    h = net.fit(x[:3], y[:3], epochs=1, batch_size=8, verbose=0)          # data set smaller than the batch
    assert np.isfinite(h.history["loss"][0])
    h = net.fit(x, y, epochs=1, batch_size=8, verbose=0)                  # 8 + ragged 3
    assert np.isfinite(h.history["loss"][0])
    with pytest.raises((DvError, ValueError)):
        net.fit(x, y, epochs=1, batch_size=9, verbose=0)                  # beyond max_batch
    with pytest.raises(ValueError):
        deblend(net, x[:, :58])                                           # wrong stamp size


def test_monte_carlo_sample_batching_is_invisible():
    """dv_infer_mc runs as many samples per decoder pass as the workspace takes; the statistics must be identical to
    one pass per sample (same noise per (stamp, sample), same fold order), for odd element counts too."""
    from debvader_amd.model import model

    x, _ = _data(3, 61)
    outs = []
    for mb in (3, 8, 64):                       # 1, 2 and 21 samples per pass
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=mb)
        eng = net._core.engine
        eng.init(seed=12)
        outs.append(eng.infer_mc(x, nsamples=10, seed=77))
    for mean, std in outs[1:]:
        np.testing.assert_array_equal(mean, outs[0][0])
        np.testing.assert_array_equal(std, outs[0][1])
    assert (outs[0][1] > 0).any()


@pytest.mark.parametrize("dtype", [0, 1])
def test_graph_replayed_small_batch_inference_equals_eager_launches(dtype):
    """BASELINE configs[4] "hipGraph-captured decode" as a product switch (dv_config.infer_graph, default off): the forward of
    a small batch replayed from a captured graph (third call of a size onwards) returns what the eager launches of a
    second engine return for the same seed; the seed - read from device memory by the replayed sampler - still changes the
    noise; and a parameter change drops the graphs (their derived weights - Winograd transforms, bf16 casts - are made by
    eager passes only), so the replay never serves stale weights."""
    from debvader_amd import engine as E

    x, _ = _data(5, 21)
    eager = E.Engine(E.make_config(max_batch=64, dtype=dtype))
    graph = E.Engine(E.make_config(max_batch=64, dtype=dtype, infer_graph=1))
    eager.init(seed=2)
    graph.init(seed=2)
    want = ("loc", "scale", "z")
    for s in (1, 2):                       # eager warm-up of this size, then the capture
        graph.infer(x, seed=s, want=want)
    for rnd in range(2):
        ref = [eager.infer(x, seed=s, want=want) for s in (7, 8)]
        rep = [graph.infer(x, seed=s, want=want) for s in (7, 8)]
        for a, b in zip(ref, rep):
            for k in want:
                np.testing.assert_array_equal(a[k], b[k])
        assert np.abs(rep[0]["z"] - rep[1]["z"]).max() > 0
        # second round: new weights in both engines - the replaying engine must notice
        k = eager.get_param("dec/convt3/kernel") * 1.5 + 0.01
        for e in (eager, graph):
            e.set_param("dec/convt3/kernel", k)
            e.set_param("enc/conv2/kernel", e.get_param("enc/conv2/kernel") * 0.5)
    eager.close()
    graph.close()


def test_deblend_sharded_single_rank_equals_deblend():
    """One rank: deblend_sharded is deblend() on the whole range (same noise seed -> bit-identical mean and stddev)."""
    from debvader_amd.deblend_cutout.deblender import deblend, deblend_sharded
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=64, seed=5)
    x, _ = _data(37, 23)
    net._core.seed_counter = 1000
    m0, d0 = deblend(net, x)
    net._core.seed_counter = 1000
    m1, s1 = deblend_sharded(net, x)
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(d0.stddev().numpy(), s1)
    net._core.seed_counter = 1000
    m2, s2, (lo, hi) = deblend_sharded(net, x, gather=False)
    assert (lo, hi) == (0, 37)
    np.testing.assert_array_equal(m0, m2)


def test_inference_chunk_of_8192_stamps_fp32_lanes_and_bf16():
    """BASELINE configs[4] quotes batch = 8192.  One fp32 launch addresses 2^30 elements (8191 stamps of the 59-pixel
    net), so the fp32 engine runs such a chunk as two forward lanes; the bf16 engine's block offsets take it whole.
    Per-stamp results do not depend on the chunking: a max_batch = 8192 engine must reproduce a max_batch = 256 engine."""
    from debvader_amd import engine as E
    from debvader_amd.data import synthetic_stamps

    base, _ = synthetic_stamps(256, seed=77)
    N = 8192 + 40
    x = np.tile(base, (N // 256 + 1, 1, 1, 1))[:N]
    for dtype in (0, 1):
        small = E.Engine(E.make_config(max_batch=256, dtype=dtype))
        small.init(3)
        ref = small.infer(x[:512], seed=9, want=("loc", "z"))
        tail = small.infer(x[N - 256:], seed=9, want=("loc",))      # rows N-256.. as rows 0.. : different noise rows
        small.close()
        big = E.Engine(E.make_config(max_batch=8192, dtype=dtype))
        big.init(3)
        out = big.infer(x, seed=9, want=("loc", "z"))
        big.close()
        assert np.isfinite(out["loc"]).all()
        # (the dense layers pick their split-K by the batch size, so fp32 agrees to rounding, not bit for bit)
        assert np.abs(out["z"][:512] - ref["z"]).max() <= (1e-5 if dtype == 0 else 2e-2) * np.abs(ref["z"]).max()
        if dtype == 0:
            assert np.abs(out["loc"][:512] - ref["loc"]).max() <= 1e-4 * np.abs(ref["loc"]).max()
        else:
            # the bf16 conv tiles hold 16 stamps of ONE pixel or of several, depending on the chunk's padding: fp32 sums
            # in another order, bf16 roundings may flip
            assert np.abs(out["loc"][:512] - ref["loc"]).max() <= 2e-2 * np.abs(ref["loc"]).max()
        assert tail["loc"].shape == (256, 59, 59, 6)


def test_tiny_inference_calls_slice_k_and_match_the_same_stamps_in_a_large_call():
    """Calls of <= 16 stamps run their deep conv layers with K sliced over workgroups (gconv2_small_splitk: a one-stamp
    layer otherwise has 1-4 workgroups walking 72 K chunks serially).  Only the order of the K sum changes: the rows must
    agree with the same stamps evaluated inside a 40-stamp call to 2e-5 of each tensor's maximum."""
    from debvader_amd import engine as E

    rng = np.random.default_rng(41)
    eng = E.Engine(E.make_config(max_batch=64))
    eng.init(seed=4)
    for name, _, _ in eng.specs:
        if name.endswith("alpha"):
            eng.set_param(name, rng.uniform(0.05, 0.3, size=eng.get_param(name).shape).astype(np.float32))
    x = rng.normal(0, 0.4, size=(40, 59, 59, 6)).astype(np.float32)
    eps = rng.normal(size=(40, 32)).astype(np.float32)
    want = ("loc", "scale", "mu", "z", "zstd")
    big = eng.infer(x, eps=eps, want=want)
    for n in (1, 5, 16):
        tiny = eng.infer(x[:n], eps=eps[:n], want=want)
        for k in want:
            err = np.abs(tiny[k] - big[k][:n]).max() / (np.abs(big[k][:n]).max() + 1e-30)
            assert err <= 2e-5, (n, k, err)
    eng.close()


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_on_device_compositing_is_bit_identical_to_the_host_composited_path(dtype):
    """DeblendField.deblend_field(on_device=True): cutout gather, network and the compositing of get_predicted_field /
    get_residual_field (field_deblender.py:99-189, :46-97) in ONE engine call with every stamp staying in HBM
    (dv_infer_cutouts_composite) against the default path - stamps to the host, then dv_scene_composite on them.  Same
    forward passes, same float64 sums in the same object order: identical bits, over several chunks (max_batch 64), with
    overlapping galaxies, a pile of 80 on one spot, stamps that hang over the field's edge when placed (even field / odd
    stamp: the pad offset differs from the window start by the reference's int() roundings) and galaxies the reference
    drops because their window leaves the field.  Also: the centre-MSE of every stamp (the reference's quality cut), the
    normalise=True form, and that only the fields came back (no stamp images in the recarray)."""
    from debvader_amd.deblend.field_deblender import DeblendField
    from debvader_amd.model import model
    from debvader_amd.training.metrics import mse

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=64, seed=3, dtype=dtype)
    rng = np.random.default_rng(23)
    for F in (160, 131):
        field = rng.normal(0, 0.4, size=(1, F, F, 6))
        half = F // 2 - 30
        d = rng.integers(-half - 6, half + 7, size=(230, 2)).astype(np.float64)     # some leave the field: dropped
        d = np.concatenate([d, np.tile(np.array([[3.0, -4.0]]), (80, 1))])          # a pile on one spot
        for normalise in (False, True):
            a = DeblendField(net, field, normalise=normalise)
            net._core.seed_counter = 900
            res = a.deblend_field(d)
            pa, ra = a.get_predicted_field(), a.get_residual_field()
            b = DeblendField(net, field, normalise=normalise)
            net._core.seed_counter = 900
            rb = b.deblend_field(d, on_device=True)
            pb, rfb = b.get_predicted_field(), b.get_residual_field()
            assert list(rb["list_idx"]) == list(res["list_idx"]) and 250 < len(rb) < 310
            np.testing.assert_array_equal(pb["predicted_mean_field"], pa["predicted_mean_field"])
            np.testing.assert_array_equal(pb["predicted_stddev_field"], pa["predicted_stddev_field"])
            np.testing.assert_array_equal(rfb, ra)
            assert np.abs(pa["predicted_mean_field"]).max() > 0 and rfb.shape == field.shape
            c0, c1 = 59 // 2 - 5, 59 // 2 + 5
            ref_mse = np.array([mse(row["cutout_images"][c0:c1, c0:c1], row["output_images_mean"][c0:c1, c0:c1]) for row in res])
            np.testing.assert_allclose(rb["mse_center"], ref_mse, rtol=1e-12, atol=0)
            assert list(rb["passed_cuts"]) == list(res["passed_cuts"])
            assert "output_images_mean" not in rb.dtype.names and "cutout_images" not in rb.dtype.names
    with pytest.raises(ValueError):
        b.deblend_field(np.array([[0.5, 1.0]]), on_device=True)                     # fractional positions: default path
    # no galaxy inside the field: the reference's dictionary of None entries (field_deblender.py:262-266), no engine call
    none = b.deblend_field(np.array([[1000.0, -1000.0]]), on_device=True)
    assert isinstance(none, dict) and none["list_idx"] is None and none["output_images_mean"] is None


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_default_deblend_field_is_one_engine_call_with_the_reference_sequences_bits(dtype, monkeypatch):
    """DeblendField.deblend_field() as the reference's caller invokes it (field_deblender.py:219-383, no engine keyword): the
    recarray of the one-call path (dv_infer_cutouts_keep: gather + cast on the GPU, float64 cutout_images assembled on the
    host beside the forward passes) against the reference's own sequence spelled out - extract_cutouts, then deblend on the
    float64 cutouts, then the per-galaxy loop with mse() - column by column, bit for bit; several chunks, galaxies the
    reference drops, both normalise modes, a non-default quality cut.  Also: the default path makes no dv_scene_extract
    call (no float64 D2H -> host cast -> H2D loop)."""
    from debvader_amd.deblend import field_deblender as fd
    from debvader_amd.deblend_cutout.deblender import deblend
    from debvader_amd.extract.extraction import extract_cutouts
    from debvader_amd.model import model
    from debvader_amd.training.metrics import mse

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=64, seed=5, dtype=dtype)
    rng = np.random.default_rng(31)
    F = 173
    field = rng.normal(0, 0.4, size=(1, F, F, 6))
    half = F // 2 - 30
    d = rng.integers(-half - 5, half + 6, size=(200, 2)).astype(np.float64)
    calls = []
    real = type(net._core.ctx).scene_extract
    for normalise in (False, True):
        a = fd.DeblendField(net, field, normalise=normalise)
        net._core.seed_counter = 400
        monkeypatch.setattr(type(net._core.ctx), "scene_extract", lambda self, *k, **kw: calls.append(1) or real(self, *k, **kw))
        res = a.deblend_field(d, mse_criterion=0.5)
        monkeypatch.undo()
        assert calls == []
        # the reference's sequence
        net._core.seed_counter = 400
        cut, list_idx = extract_cutouts(field, F, d, 59, 6, ctx=net._core.ctx)
        mean, dist = deblend(net, cut[list_idx], normalise=normalise)
        std = dist.stddev().numpy()
        assert 150 < len(list_idx) < 200 and list(res["list_idx"]) == list_idx
        c0, c1 = 59 // 2 - 5, 59 // 2 + 5
        for i, k in enumerate(list_idx):
            np.testing.assert_array_equal(res["cutout_images"][i], cut[k])
            np.testing.assert_array_equal(res["output_images_mean"][i], mean[i])
            np.testing.assert_array_equal(res["output_images_stddev"][i], std[i])
            assert res["galaxy_distances_to_center_x"][i] == d[k][0] and res["galaxy_distances_to_center_y"][i] == d[k][1]
            assert bool(res["passed_cuts"][i]) == (not mse(cut[k, c0:c1, c0:c1], mean[i, c0:c1, c0:c1]) > 0.5)
            assert np.array_equal(res["shifts"][i], [0, 0]) and not np.any(res["epistemic_uncertainty"][i])
        assert res["cutout_images"][0].dtype == np.float64 and res["output_images_mean"][0].dtype == np.float32
        assert a.nb_of_detected_objects == [200] and a.nb_of_deblended_galaxies == [len(list_idx)]
    # caller-supplied cutouts keep the reference's branch (:254-258): every row is deblended, list_idx counts them
    rb = a.deblend_field(d[:7], cutout_images=cut[list_idx][:7])
    assert list(rb["list_idx"]) == list(range(7)) and rb["output_images_mean"][0].shape == (59, 59, 6)


def test_on_device_pass_refuses_what_it_cannot_honour_and_keeps_fields_and_recarray_together():
    """deblend_field(on_device=True) must not silently drop arguments of the reference's signature, and the
    device-composited fields must never be served for a recarray they do not belong to."""
    from debvader_amd.deblend.field_deblender import DeblendField
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=32, seed=2)
    rng = np.random.default_rng(5)
    F = 140
    field = rng.normal(0, 0.3, size=(1, F, F, 6))
    d = np.array([[0.0, 0.0], [10.0, -12.0], [-20.0, 5.0]])
    a = DeblendField(net, field)
    with pytest.raises(NotImplementedError):
        a.deblend_field(d, on_device=True, optimise_positions=True)
    with pytest.raises(ValueError, match="cutout_images"):
        a.deblend_field(d, on_device=True, cutout_images=np.zeros((3, 59, 59, 6)))
    with pytest.raises(ValueError, match="field_image"):
        a.deblend_field(d, on_device=True, field_image=field + 1.0)
    assert a.res_deblend is None
    ra = a.deblend_field(d, on_device=True, field_image=field.copy())          # an equal field is the object's own field
    dev_mean = a.get_predicted_field()["predicted_mean_field"]
    assert np.abs(dev_mean).max() > 0
    # (1) a default-path call that returns early leaves recarray AND fields of the on-device pass in place
    assert a.deblend_field(np.array([[1000.0, 1000.0]]))["list_idx"] is None
    assert a.res_deblend is ra
    np.testing.assert_array_equal(a.get_predicted_field()["predicted_mean_field"], dev_mean)
    np.testing.assert_array_equal(a.get_residual_field(), a.get_residual_field(ra))
    # (2) an on-device early return does the same
    assert a.deblend_field(np.array([[1000.0, 1000.0]]), on_device=True)["list_idx"] is None
    np.testing.assert_array_equal(a.get_predicted_field()["predicted_mean_field"], dev_mean)
    # (3) a default-path pass replaces both: the fields now come from ITS stamps
    net._core.seed_counter = 77
    rd = a.deblend_field(d[:2])
    assert a.res_deblend is rd and "output_images_mean" in rd.dtype.names
    assert not np.array_equal(a.get_predicted_field()["predicted_mean_field"], dev_mean)
    # (4) an on-device recarray without its object: a clear error instead of a KeyError inside the compositing
    with pytest.raises(ValueError, match="on_device"):
        a.get_predicted_field(ra)
    with pytest.raises(ValueError, match="on_device"):
        DeblendField(net, field).get_residual_field(ra)


def test_deblend_field_cutouts_equals_extract_then_deblend_bit_for_bit():
    """DeblendField's extract_cutouts -> deblend pair (field_deblender.py:260-274) as one engine call with the gather and
    the float32 cast on the GPU (dv_infer_cutouts): same cast, same kernels, same noise numbering - identical results,
    on both sides of the pipelined path's size threshold and for a tiny call; windows leaving the field are refused."""
    from debvader_amd._lib import DvError
    from debvader_amd.deblend_cutout.deblender import deblend, deblend_field_cutouts
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=128, seed=3)
    ctx = net._core.ctx
    rng = np.random.default_rng(17)
    F = 300
    field = rng.normal(0, 0.4, size=(F, F, 6))
    for n in (5, 200, 128 * 3 + 11):
        starts = rng.integers(0, F - 59 + 1, size=(n, 2)).astype(np.int32)
        cut = ctx.scene_extract(field, starts, 59)
        np.testing.assert_array_equal(cut[0], field[starts[0, 0]:starts[0, 0] + 59, starts[0, 1]:starts[0, 1] + 59])
        net._core.seed_counter = 500
        m0, d0 = deblend(net, cut)
        net._core.seed_counter = 500
        m1, d1 = deblend_field_cutouts(net, field, starts)
        np.testing.assert_array_equal(m1, m0)
        np.testing.assert_array_equal(d1.stddev().numpy(), d0.stddev().numpy())
    with pytest.raises(DvError):
        deblend_field_cutouts(net, field, np.array([[F - 58, 0]], np.int32))
    # streaming consumer: the same numbers chunk by chunk, in order, nothing copied by the library
    got_m, got_s, firsts = [], [], []

    def consume(first, mean, std):
        firsts.append(first)
        got_m.append(mean.copy())
        got_s.append(std.copy())

    net._core.seed_counter = 500
    assert deblend_field_cutouts(net, field, starts, on_chunk=consume) is None
    assert firsts == sorted(firsts) and firsts[0] == 0 and len(firsts) == 4
    np.testing.assert_array_equal(np.concatenate(got_m), m0)
    np.testing.assert_array_equal(np.concatenate(got_s), d0.stddev().numpy())

    def broken(first, mean, std):
        raise RuntimeError("consumer failed")

    with pytest.raises(RuntimeError):
        deblend_field_cutouts(net, field, starts, on_chunk=broken)
    m2, _ = deblend_field_cutouts(net, field, starts[:3])          # the engine is usable afterwards
    assert np.isfinite(m2).all()


def test_infer_cutouts_stream_hands_out_every_chunk_at_its_global_offset():
    """The chunk consumer is one sink of the implementation behind all field-sourced calls: for a call of more than two
    chunks, consumer(first, ...) gets first = the chunk's global stamp number, chunk after chunk without gaps, and the
    stamps are infer_cutouts' for the same seed, bit for bit."""
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=128, seed=3)
    eng = net._core.engine
    rng = np.random.default_rng(23)
    F, n = 200, 128 * 4 + 37
    field = rng.normal(0, 0.4, size=(F, F, 6))
    starts = rng.integers(0, F - 59 + 1, size=(n, 2)).astype(np.int32)
    ref = eng.infer_cutouts(field, starts, seed=91)
    chunks = []
    eng.infer_cutouts_stream(field, starts, lambda first, mean, std: chunks.append((first, mean.copy(), std.copy())), seed=91)
    assert [c[0] for c in chunks] == [0, 128, 256, 384, 512]
    assert [len(c[1]) for c in chunks] == [128, 128, 128, 128, 37]
    for first, mean, std in chunks:
        np.testing.assert_array_equal(mean, ref["loc"][first:first + len(mean)])
        np.testing.assert_array_equal(std, ref["scale"][first:first + len(std)])


def test_config0_plumbing_1000_stamps_batch_5_and_256():
    """BASELINE configs[0] / SURVEY 8(d) "Config 1 (plumbing)": 1000 synthetic stamps of the survey's generator, latent 32,
    one epoch of net.fit at the reference's default batch 5 (train.py:88) and at 256, through the same surface
    train_network uses (train.py:27-37).  Step counts, History keys and the ELBO of the trained weights against the
    oracle (same weights, same eps) are checked; the oracle's CPU run of this configuration is bench.py's cpu_baseline."""
    from debvader_amd.model import model
    from debvader_amd.training.metrics import vae_loss
    from oracle import vae_oracle as vo

    x, y = _data(1000, 0)
    xv, yv = _data(64, 7)
    for batch, steps in ((5, 200), (256, 4)):
        net, _, _, _ = model.create_model_vae(**ARCH, max_batch=256, seed=11)
        net.compile(optimizer=model.Adam(learning_rate=1e-4), loss=vae_loss, metrics=["mse"])
        hist = net.fit(x, y, epochs=1, batch_size=batch, verbose=0, shuffle=True, validation_data=(xv, yv))
        eng = net._core.engine
        assert eng.iterations == steps                      # 1000 / 256: three full batches and one of 232
        assert sorted(hist.history) == ["loss", "mse", "val_loss", "val_mse"]
        assert all(len(v) == 1 and np.isfinite(v).all() for v in hist.history.values())
        # the trained weights, evaluated by the engine and by the oracle on the same 5 stamps with the same noise
        p = {k: v.astype(np.float64) for k, v in eng.get_params().items()}
        eps = np.random.default_rng(3).normal(size=(5, 32)).astype(np.float32)
        eng.upload(1, x[:5], y[:5])
        out = eng.eval_step(1, first=0, B=5, eps=eps)
        arch = vo.Arch()
        c = vo.forward(arch, p, x[:5].astype(np.float64), eps.astype(np.float64), training=False)
        r = vo.losses(arch, c, y[:5].astype(np.float64))
        for k in ("loss", "nll_mean", "kl_reg"):
            assert abs(out[k] - r[k]) <= 1e-4 * abs(r[k]) + 1e-7, (batch, k, out[k], r[k])


@pytest.mark.gpu
def test_multi_rank_bench_launch_rehearsed_on_one_gpu():
    """The driver's N > 1 launch line with the REAL engine: `python -m torch.distributed.run --nproc-per-node 2 bench.py
    --gpus 2`.  A build box has one GPU and RCCL refuses two ranks on one device, so DV_DEBUG_SAME_GPU=1 opens device 0
    on every rank and DV_DEBUG_FAKE_PEERS=1 gives each rank a one-rank communicator (the gradients are not summed: the
    numbers mean nothing).  What runs for real: the torch-free rendezvous beside torchrun's own store, rank 0's RCCL id
    reaching every rank, a context that believes in two ranks (system-scope ordering events, global batch 2 x 256 in the
    loss scale and the BN statistics, collectives on the comm stream), the barriers and the MAX over ranks, ONE JSON
    line from rank 0, and a clean exit of every process."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    # the rehearsal hooks exist in the DEVELOPMENT library only (round 6): with the product library the same variables are
    # ignored (one line on stderr), so a stray one cannot turn a job into a rehearsal
    env.update({"DV_DEBUG_SAME_GPU": "1", "DV_DEBUG_FAKE_PEERS": "1",
                "DEBVADER_AMD_LIB": os.path.join(root, "debvader_amd", "lib", "libdebvader_hip_debug.so")})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29517", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "3",
           "--no-roofline", "--no-secondary", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 512 and d["config"]["parallelism"] == "dp2"
    assert d["steps"] == 8 and np.isfinite(d["last_loss"])
    # ... and the line says what it is (an environment variable left over from a rehearsal used to print
    # "dp2" numbers that meant nothing, silently): no value, a rehearsal tag, and the evidence - RCCL reports ONE rank per
    # communicator, both ranks sit on the same PCI device - so `verified` is false; the warning went to stderr
    mr = d["multi_rank"]
    assert d["value"] is None and d["rehearsal"] is True and d["rehearsal_stamps_per_s"] > 0
    assert mr["rehearsal"] is True and mr["verified"] is False and mr["rccl_ranks"] == [1, 1] and mr["distinct_devices"] == 1
    assert mr["collectives_per_step"] >= 4 and mr["comm_ms_per_step"] > 0 and mr["exposed_comm_ms_per_step"] >= 0
    assert "DV_DEBUG_FAKE_PEERS is set" in r.stderr and "REHEARSAL" in r.stderr


def test_comm_timing_and_comm_info_on_a_one_rank_communicator():
    """dv_ctx_comm_info / dv_comm_prof_*: with DV_FORCE_COMM=1 (a one-rank RCCL communicator on this GPU) a train step issues
    its collectives - BN sums, loss sums, three gradient buckets - on the comm stream; the profile counts them and their
    time, the info reports what ncclCommCount says."""
    import json
    import os
    import subprocess
    import sys

    code = r'''
import sys, json
sys.path.insert(0, %r)
from debvader_amd import engine as E
from debvader_amd.data import synthetic_stamps
x, y = synthetic_stamps(64, seed=3)
ctx = E.default_context()
eng = E.Engine(E.make_config(max_batch=32))
eng.init(seed=4); eng.optimizer_reset(1e-4); eng.upload(0, x, y)
eng.train_steps(0, 0, 32, 2, seed=7)
ctx.comm_prof(True)
eng.train_steps(0, 0, 32, 4, seed=9)
p = ctx.comm_prof_read()
ctx.comm_prof(False)
eng.train_steps(0, 0, 32, 2, seed=11)
q = ctx.comm_prof_read()
print(json.dumps(dict(info=ctx.comm_info(), p=p, q=q)))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for force in ("", "1"):
        env = dict(os.environ)
        env.pop("DV_FORCE_COMM", None)
        if force:
            env["DV_FORCE_COMM"] = "1"
        r = subprocess.run([sys.executable, "-c", code % root], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[force] = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = res[""], res["1"]
    assert a["info"]["comm_ranks"] == 0 and a["p"]["collectives"] == 0 and a["info"]["rehearsal"] is False
    assert len(a["info"]["bus_id"]) >= 7
    assert b["info"]["comm_ranks"] == 1 and b["info"]["comm_rank"] == 0
    # per train step: the next batch's BN sums, the loss sums, three gradient buckets
    assert b["p"]["collectives"] >= 4 * 4 and b["p"]["comm_ms"] > 0 and b["p"]["waits"] >= 4 and b["p"]["exposed_ms"] >= 0
    assert b["q"]["collectives"] == 0                       # switched off again: nothing recorded

