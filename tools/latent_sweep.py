"""Step time of the reference architecture (59 x 59 x 6, filters 32 ... 256) at several latent sizes, both engines: the
bench's measurement (resident synthetic stamps, random-init weights, train_steps between two device drains) with
latent_dim varied.  One JSON line per (dtype, latent_dim).
usage: latent_sweep.py [--batch 256] [--steps 50] [--warmup 10] [--latents 32,64,65,128,256] [--dtypes f32,bf16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--latents", default="32,64,65,128,256")
    ap.add_argument("--dtypes", default="f32,bf16")
    args = ap.parse_args()
    from debvader_amd import engine as E
    from debvader_amd.data import bench_stamps

    B = args.batch
    x, y, _ = bench_stamps(4 * B, seed=1000)
    ctx = E.default_context()
    for dt in args.dtypes.split(","):
        for d in (int(v) for v in args.latents.split(",")):
            eng = E.Engine(E.make_config(latent_dim=d, max_batch=B, dtype=1 if dt == "bf16" else 0), ctx)
            eng.init(seed=0)
            eng.upload(0, x, y)
            eng.optimizer_reset(1e-4)
            eng.train_steps(0, 0, B, args.warmup, seed=1)
            ctx.sync()
            t0 = time.perf_counter()
            scal = eng.train_steps(0, 0, B, args.steps, seed=100)
            ctx.sync()
            sec = (time.perf_counter() - t0) / args.steps
            print(json.dumps({"dtype": dt, "latent_dim": d, "batch": B, "steps": args.steps, "step_ms": round(1e3 * sec, 4),
                              "stamps_per_s": round(B / sec, 1), "loss": scal["loss"],
                              "finite": bool(np.isfinite(scal["loss"]))}), flush=True)
            eng.close()


if __name__ == "__main__":
    main()
