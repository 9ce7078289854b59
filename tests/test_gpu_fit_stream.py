"""fit() / evaluate() on data streamed from host memory (device_data_budget, Engine.open_stream): the engine gathers every
step's rows into pinned memory and copies them into a four-deep device ring while earlier steps run.  The same rows in the
same order reach the same kernels as on a resident slot, so every result must be bit-identical to resident training:
weights, both Adam slots, the iteration counter, the BatchNorm moving statistics (parameters of the model) and History."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOY = dict(input_shape=(13, 13, 4), latent_dim=8, filters=[8, 16], kernels=[3, 3])
REF = dict(input_shape=(59, 59, 6), latent_dim=32, filters=[32, 64, 128, 256], kernels=[3, 3, 3, 3])


def _data(n, seed, arch, dtype=np.float32):
    from debvader_amd.data import synthetic_stamps

    h, _, c = arch["input_shape"]
    return synthetic_stamps(n, seed=seed, size=h, nb=c, dtype=dtype)


def _net(arch, batch, dtype="float32", seed=4):
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**arch, max_batch=batch, seed=seed, dtype=dtype)
    net.compile(optimizer=model.Adam(learning_rate=1e-3), metrics=["mse"])
    net._core.seed_counter = 1000          # the noise seeds of the steps (drawn from the OS by default)
    return net


def _state(net):
    eng = net._core.engine
    out = {"iterations": np.array(eng.iterations)}
    for i, (name, _, trainable) in enumerate(eng.specs):      # (the BN moving statistics are parameters of the model)
        out["p/" + name] = eng.get_param(i)
        if trainable:
            out["m/" + name] = eng.get_slot(i, 0)
            out["v/" + name] = eng.get_slot(i, 1)
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _fit_pair(arch, batch, n, nv, epochs, dtype):
    x, y = _data(n, 11, arch)
    xv, yv = _data(nv, 12, arch)
    runs = []
    for budget in (None, 0):
        net = _net(arch, batch, dtype)
        h = net.fit(x, y, batch_size=batch, epochs=epochs, verbose=0, shuffle=True, validation_data=(xv, yv),
                    shuffle_seed=7, device_data_budget=budget)
        runs.append((net, h, net._core.engine.data_info(0), net._core.engine.data_info(1)))
    (nr, hr, ir, _), (ns, hs, is_, ivs) = runs
    assert ir["mode"] == 1, "a set that fits in HBM must stay resident by default"
    stamp_bytes = 4 * int(np.prod(arch["input_shape"]))
    assert is_["mode"] == 2 and ivs["mode"] == 2
    assert is_["h2d_bytes"] == epochs * n * 2 * stamp_bytes
    assert ivs["h2d_bytes"] == epochs * nv * 2 * stamp_bytes
    assert hr.history == hs.history and len(hs.history["val_loss"]) == epochs
    _assert_same(_state(nr), _state(ns))


def test_streamed_fit_bit_identical_to_resident_fp32_toy():
    """3 shuffled epochs of 11 steps (a ragged last batch of 3), more steps than the ring is deep, with validation"""
    _fit_pair(TOY, batch=8, n=83, nv=21, epochs=3, dtype="float32")


def test_streamed_fit_bit_identical_to_resident_bf16_reference_arch():
    """bf16 engine at the reference architecture and batch 256: its comm stream normalises the next step's input ahead
    (bn_prefetch -> bf_input into xh_alt), one of the readers the ring must wait for before it overwrites an entry"""
    _fit_pair(REF, batch=256, n=256 * 10 + 40, nv=300, epochs=3, dtype="bf16")


def test_streamed_float64_and_memmap_match_resident_float32_cast(tmp_path):
    n, batch = 45, 8
    x64, y64 = _data(n, 5, TOY, dtype=np.float64)
    x64 = x64 * (1.0 + 1e-9)                   # values that are not float32 already: the cast must round like numpy's
    x32, y32 = x64.astype(np.float32), y64.astype(np.float32)
    path = tmp_path / "x.f32"
    mm = np.memmap(path, dtype=np.float32, mode="w+", shape=x32.shape)
    mm[:] = x32
    mm.flush()
    del mm
    xm = np.memmap(path, dtype=np.float32, mode="r", shape=x32.shape)

    def run(x, y, budget):
        net = _net(TOY, batch)
        h = net.fit(x, y, batch_size=batch, epochs=2, verbose=0, shuffle_seed=3, device_data_budget=budget)
        assert net._core.engine.data_info(0)["mode"] == (2 if budget == 0 else 1)
        return h.history, _state(net)

    ref_h, ref_s = run(x32, y32, None)
    for x, y in ((x64, y64), (xm, y32)):
        h, s = run(x, y, 0)
        assert h == ref_h
        _assert_same(s, ref_s)


def test_streamed_evaluate_matches_resident():
    x, y = _data(29, 8, TOY)
    out = []
    for budget in (None, 0):
        net = _net(TOY, 8)
        net._core.seed_counter = 50
        out.append(net.evaluate(x, y, batch_size=8, device_data_budget=budget))
        assert net._core.engine.data_info(1)["mode"] == (2 if budget == 0 else 1)
    assert out[0] == out[1]


def test_streamed_fit_after_a_callback_raised_matches_a_fresh_run():
    """A host-side exception in on_epoch_end leaves the streamed slot reusable: the next fit() completes and trains
    exactly as a model whose first fit() ended normally after that epoch."""
    x, y = _data(50, 9, TOY)

    class Boom:
        def on_epoch_end(self, epoch, logs):
            raise KeyError("callback failed")

    a = _net(TOY, 8)
    with pytest.raises(KeyError):
        a.fit(x, y, batch_size=8, epochs=3, verbose=0, callbacks=[Boom()], shuffle_seed=1, device_data_budget=0)
    ha = a.fit(x, y, batch_size=8, epochs=2, verbose=0, shuffle_seed=2, device_data_budget=0)

    b = _net(TOY, 8)
    b.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle_seed=1, device_data_budget=0)
    hb = b.fit(x, y, batch_size=8, epochs=2, verbose=0, shuffle_seed=2, device_data_budget=0)
    assert ha.history == hb.history
    _assert_same(_state(a), _state(b))
