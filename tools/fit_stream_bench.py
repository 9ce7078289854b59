"""net.fit() throughput with the training set resident in HBM against the same set streamed from host memory
(device_data_budget=0: rows gathered into pinned memory and copied to the device ring while earlier steps run).

59x59x6 stamps, batch 256, the reference architecture, fp32 and bf16 engines; per row: stamps/s of the whole fit() call
(the resident upload included), of its last epoch alone, and the host time per step spent in train_step_async (the
gather of 2 x 256 rows into pinned staging plus queueing the copy and the step) - the part of a step the host, not the
GPU, pays for streaming.

    python tools/fit_stream_bench.py [--stamps 20480] [--epochs 2] [--out profiles/r07_fit_stream.txt]
    python tools/fit_stream_bench.py --trace-epoch      # one streamed fp32 epoch, for rocprofv3 --kernel-trace
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from debvader_amd.data import synthetic_stamps  # noqa: E402
from debvader_amd.model import model  # noqa: E402

B = 256


class _EpochClock:
    def __init__(self):
        self.t = [time.perf_counter()]

    def on_epoch_end(self, epoch, logs):
        self.t.append(time.perf_counter())


def run(x, y, dtype, budget, epochs):
    net, _, _, _ = model.create_model_vae((59, 59, 6), 32, [32, 64, 128, 256], [3, 3, 3, 3], max_batch=B, seed=1,
                                          dtype=dtype)
    net.compile(optimizer=model.Adam(learning_rate=1e-4), metrics=["mse"])
    net.fit(x[:4 * B], y[:4 * B], batch_size=B, epochs=1, verbose=0, device_data_budget=budget)     # warm-up
    eng = net._core.engine
    host = []
    step = eng.train_step_async

    def timed(*a, **k):
        t = time.perf_counter()
        step(*a, **k)
        host.append(time.perf_counter() - t)

    eng.train_step_async = timed
    clock = _EpochClock()
    t0 = time.perf_counter()
    h = net.fit(x, y, batch_size=B, epochs=epochs, verbose=0, callbacks=[clock], device_data_budget=budget)
    dt = time.perf_counter() - t0
    info = eng.data_info(0)
    n = x.shape[0]
    last = clock.t[-1] - clock.t[-2]
    host = np.array(host[len(host) // 4:]) * 1e3       # steady state
    eng.close()
    return dict(fit=epochs * n / dt, last_epoch=n / last, host_ms=float(np.median(host)), host_p90=float(np.percentile(host, 90)),
                mode=info["mode"], h2d_gb=info["h2d_bytes"] / 1e9, loss=h.history["loss"][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamps", type=int, default=20480)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-epoch", action="store_true", help="one streamed fp32 epoch of 16 steps (profiler run)")
    a = ap.parse_args()
    base_x, base_y = synthetic_stamps(2048, seed=1)
    if a.trace_epoch:
        net, _, _, _ = model.create_model_vae((59, 59, 6), 32, [32, 64, 128, 256], [3, 3, 3, 3], max_batch=B, seed=1)
        net.compile(optimizer=model.Adam(learning_rate=1e-4))
        t0 = time.perf_counter()
        net.fit(base_x[:16 * B // 2], base_y[:16 * B // 2], batch_size=B, epochs=2, verbose=0, device_data_budget=0)
        print(f"streamed fp32: 2 epochs of 8 steps in {(time.perf_counter() - t0) * 1e3:.1f} ms")
        return
    reps = -(-a.stamps // base_x.shape[0])
    x = np.tile(base_x, (reps, 1, 1, 1))[:a.stamps]
    y = np.tile(base_y, (reps, 1, 1, 1))[:a.stamps]
    lines = [f"fit() stamps/s, 59x59x6, batch {B}, {a.stamps} stamps, {a.epochs} epochs, shuffled; "
             f"host = median (p90) host ms per step inside train_step_async, steady state",
             f"{'engine':6} {'data':9} {'fit() stamps/s':>15} {'last epoch':>11} {'host ms':>8} {'(p90)':>7} {'H2D GB':>7}  loss"]
    res = {}
    for dtype in ("float32", "bf16"):
        for name, budget in (("resident", None), ("streamed", 0)):
            r = run(x, y, dtype, budget, a.epochs)
            res[dtype, name] = r
            lines.append(f"{dtype:6} {name:9} {r['fit']:15.0f} {r['last_epoch']:11.0f} {r['host_ms']:8.3f} {r['host_p90']:7.3f} "
                         f"{r['h2d_gb']:7.2f}  {r['loss']:.6f}  (slot mode {r['mode']})")
            print(lines[-1], flush=True)
    for dtype in ("float32", "bf16"):
        rr, rs = res[dtype, "resident"], res[dtype, "streamed"]
        lines.append(f"{dtype}: streamed / resident last epoch {rs['last_epoch'] / rr['last_epoch']:.3f}, "
                     f"whole fit() {rs['fit'] / rr['fit']:.3f}; gather + queue {rs['host_ms'] - rr['host_ms']:.3f} ms per step "
                     f"more host time than resident")
        print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
