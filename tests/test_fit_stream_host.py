"""Host logic of streamed training (fit / evaluate with device_data_budget), on CPU with a recording stand-in for the engine:
where the rows go (resident or streamed) for an explicit budget, for 0 and for the default against a faked device-memory
report; that every rank of 1, 3 and 8 asks the engine for exactly its home rows, each once per epoch, in the order the
resident path addresses them; and that streaming a float64 set through fit() never materialises a copy of it."""
import tracemalloc
import types

import numpy as np
import pytest

from debvader_amd.model import model as M

GiB = 1 << 30


class _Ctx:
    def __init__(self, rank, world, mem=None):
        self.rank, self.world = rank, world
        if mem is not None:
            self.mem_info = lambda: mem

    def allreduce(self, v):
        return list(v)


class _Engine:
    """Resident slots keep a float32 copy (as dv_data_upload does); streamed slots only a reference to the arrays.
    Every training step records the GLOBAL row numbers it reads."""

    def __init__(self, max_batch, fail_upload=False):
        self.max_batch, self.fail_upload = max_batch, fail_upload
        self.slots, self.rows, self.evals, self.tickets, self.specs = {}, [], [], set(), []

    def upload(self, slot, x, y):
        if self.fail_upload:
            raise RuntimeError("libdebvader_hip status 2: hipMalloc(data x): out of memory")
        x = np.asarray(x, np.float32)
        self.slots[slot] = ("resident", np.array(x), np.array(np.asarray(y, np.float32)))
        return x.shape[0]

    def open_stream(self, slot, x, y):
        assert isinstance(x, np.ndarray) and x.dtype in (np.float32, np.float64)
        self.slots[slot] = ("streamed", x, y)
        return x.shape[0]

    def data_info(self, slot):
        if slot not in self.slots:
            return {"mode": 0, "n": 0, "h2d_bytes": 0}
        kind, x, _ = self.slots[slot]
        return {"mode": 1 if kind == "resident" else 2, "n": x.shape[0], "h2d_bytes": 0}

    def _global(self, slot, idx=None, first=0, B=None):
        kind, x, _ = self.slots[slot]
        r = np.asarray(idx, np.int64) if idx is not None else np.arange(first, first + B)
        if kind == "resident":                                   # the test data encode their global row number
            return (np.asarray(x[r][:, 0, 0, 0]) // 4).astype(np.int64)
        return r

    def train_step_async(self, ticket, slot, idx=None, first=0, B=None, global_batch=None, seed=0):
        assert ticket not in self.tickets
        self.tickets.add(ticket)
        self.rows.append(self._global(slot, idx, first, B))

    def step_result(self, ticket):
        self.tickets.remove(ticket)
        return {"loss": 1.0, "nll_mean": 0.9, "kl_reg": 0.1, "mse": 0.5}

    def eval_step(self, slot, idx=None, first=0, B=None, global_batch=None, eps=None, seed=0):
        self.evals.append(self._global(slot, idx, first, B))
        return {"loss": 2.0, "nll_mean": 1.9, "kl_reg": 0.1, "mse": 0.7}


def _net(rank=0, world=1, max_batch=64, mem=None, fail_upload=False):
    core = types.SimpleNamespace(
        engine=_Engine(max_batch, fail_upload), ctx=_Ctx(rank, world, mem), compiled=True, shuffle_base=99,
        upload_keys={}, init_seed=7, cfg=types.SimpleNamespace(kl_multiplicity=2))
    core.next_seed = lambda: 1
    net = M.VAENet(core, M.Encoder(core, "encoder"), M.Decoder(core, "decoder"))
    net._metrics = ["mse"]
    return net, core


def _xy(n, dtype=np.float32):
    x = np.arange(n * 4, dtype=dtype).reshape(n, 2, 2, 1)
    return x, x + 1


def _mode(core, slot=0):
    return core.engine.slots[slot][0]


def test_explicit_budget_and_zero():
    x, y = _xy(40)
    need = 2 * 40 * 16                          # x and y as float32, 16 bytes per stamp
    for budget, want in ((need, "resident"), (need - 1, "streamed"), (0, "streamed"), (10 * GiB, "resident")):
        net, core = _net()
        net.fit(x, y, batch_size=8, epochs=1, verbose=0, device_data_budget=budget)
        assert _mode(core) == want, budget
    # validation rows are charged against what the training rows left of the budget
    net, core = _net()
    net.fit(x, y, batch_size=8, epochs=1, verbose=0, validation_data=_xy(10), device_data_budget=need + 2 * 10 * 16 - 1)
    assert (_mode(core, 0), _mode(core, 1)) == ("resident", "streamed")
    net, core = _net()
    net.evaluate(x, y, batch_size=8, device_data_budget=0)
    assert _mode(core, 1) == "streamed"


def test_default_budget_against_device_memory():
    big = 64 * GiB
    reserve = M.VAENet._device_reserve(big)
    assert reserve == 2 * GiB
    x, y = _xy(40)
    need = 2 * 40 * 16
    # plenty of memory: resident
    net, core = _net(mem=(big, big))
    assert net._placement(0, need, 16, None) == "resident"
    # inside the reserve but within free memory: the resident upload is tried first ...
    net, core = _net(mem=(reserve + need - 1, big))
    assert net._placement(0, need, 16, None) == "try"
    net.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert _mode(core) == "resident"
    # ... and streamed when it fails
    net, core = _net(mem=(reserve + need - 1, big), fail_upload=True)
    net.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert _mode(core) == "streamed"
    # more than the free memory: streamed without trying
    net, core = _net(mem=(need - 1, big), fail_upload=True)
    assert net._placement(0, need, 16, None) == "stream"
    net.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert _mode(core) == "streamed"
    # the slot's own resident rows are freed before the new ones are allocated: a second fit() of the same set stays
    net, core = _net(mem=(need - 1, big))
    core.engine.upload(0, x, y)
    assert net._placement(0, need, 16, None) == "try"
    # explicit budgets ignore the device report
    assert net._placement(0, need, 16, 0) == "stream"


@pytest.mark.parametrize("world", [1, 3, 8])
def test_every_rank_streams_exactly_its_home_rows_in_resident_order(world):
    n, nv, batch, epochs = 109, 45, 16, 3
    x, y = _xy(n)
    xv, yv = _xy(nv)
    union = []
    for r in range(world):
        got = {}
        for budget in (None, 0):
            net, core = _net(r, world)
            net.fit(x, y, batch_size=batch, epochs=epochs, verbose=0, validation_data=(xv, yv), shuffle_seed=5,
                    device_data_budget=budget)
            got[budget] = core.engine
        res, st = got[None], got[0]
        assert _mode(types.SimpleNamespace(engine=st)) == "streamed"
        assert len(st.rows) == len(res.rows)
        for a, b in zip(res.rows, st.rows):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(res.evals, st.evals):
            np.testing.assert_array_equal(a, b)
        home, _ = M.VAENet._home_rows(n, batch, r, world)
        steps = len(st.rows) // epochs
        for e in range(epochs):
            rows = np.concatenate(st.rows[e * steps:(e + 1) * steps])
            np.testing.assert_array_equal(np.sort(rows), np.sort(home))        # each home row once per epoch
        union.append(home)
    np.testing.assert_array_equal(np.sort(np.concatenate(union)), np.arange(n))


def test_streamed_float64_fit_makes_no_copy_of_the_set():
    n, batch = 4000, 32
    x = np.random.default_rng(0).standard_normal((n, 13, 13, 4))            # float64, 21.6 MB
    y = x + 1.0
    batch_bytes = 2 * batch * 13 * 13 * 4 * 4
    net, core = _net(max_batch=batch)
    tracemalloc.start()
    try:
        net.fit(x, y, batch_size=batch, epochs=2, verbose=0, device_data_budget=0)
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    assert _mode(core) == "streamed" and core.engine.slots[0][1] is x
    assert peak < 4 * batch_bytes, f"fit() allocated {peak} bytes; a batch is {batch_bytes}"
