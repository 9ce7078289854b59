"""CPU helper of the trajectory tests (TEST INFRASTRUCTURE): training beyond the first step, restated over the oracle.

Plain numpy over oracle/vae_oracle.py (and its bf16-rounding variant); nothing of the product is imported here.  Three uses:
  * teacher-forced steps - one oracle step evaluated FROM A GIVEN STATE (parameters, both Adam slots, the step counter),
    so that a trained engine can be checked step by step without anything cascading (evaluate / adam_from / moving_after);
  * the power of such a comparison - how far an output moves when one group of tensors is held one step stale
    (groups / stale_effects);
  * free-running trajectories - the queued steps and Keras' fit loop (train.py:27-37: per-epoch permutation, ragged last
    batch, batch-size-weighted epoch means, validation in inference mode after the epoch's updates), in float64 and, for the
    float32 floor of such a comparison, in numpy float32 (run_steps / fit_loop / vae_fit).
"""
import numpy as np

from oracle import vae_oracle as vo
from oracle import vae_oracle_bf16 as vb

SCALARS = ("loss", "nll_mean", "kl_reg", "mse")
MSE_STREAM = 0x4D534500          # the Philox stream of the sample the Keras "mse" metric is taken against (one rank)

# the learning rates, output bounds and seeds of tests/test_trajectory_host.py (premises) and tests/test_gpu_trajectory.py
TEACHER = {"fp32": dict(lr=1e-3, bound=2e-4, sigma_bias=0.0, bf16=False),
           "bf16": dict(lr=1e-2, bound=1e-2, sigma_bias=0.3, bf16=True)}
TEACHER_SEED = 41
NEED = 5.0                  # a stale group must move t or loc by this many bounds
FREE_LR = 1e-4
QUEUE = dict(seed=70, n=18, first=0, B=6, steps=6, run_seed=900, eval_seed=977)
FIT = dict(seed=80, n=12, nv=7, batch_size=5, epochs=2, shuffle_seed=11, seed0=5000)


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-30))


def nets():
    """The smallest nets that take the kernels in question: T8 (direct, strip and stride-2 kernels, both SAME-pad cases, odd
    crop) and T32 (>= 32 channels on both sides of every stride-1 layer: the Winograd kernels; the bf16 engine's form)."""
    return {"T8": vo.Arch(input_shape=(13, 13, 4), latent_dim=8, filters=(8, 16), kernels=(3, 3)),
            "T32": vo.Arch(input_shape=(13, 13, 4), latent_dim=8, filters=(32, 64), kernels=(3, 3))}


def case(arch, n, seed, sigma_bias=0.0):
    """Parameters (float32 values in float64), n stamps and labels: tests/test_gpu_parity.py::_case without its eps."""
    rng = np.random.default_rng(seed)
    p = vo.init_params(arch, seed=seed + 1, perturb=0.05)
    p["dec/head/bias"][arch.nb:] += sigma_bias
    H, W, C = arch.input_shape
    x = rng.normal(0, 0.4, size=(n, H, W, C)).astype(np.float32)
    y = np.abs(rng.normal(0, 0.4, size=(n, H, W, C))).astype(np.float32)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}, x, y


def teacher_schedule(arch, seed):
    """The five teacher-forced steps: (first row, stamps, eps, decoder trained).  Three different batches of 6 stamps out
    of 18, one per step in turn - no step repeats the input of the one before - the third step ragged (5 stamps); stage 1 for
    steps 1-3, stage 2 (decoder frozen, fresh optimizer) for steps 4-5."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(5):
        B = 5 if k == 2 else 6
        out.append(((k % 3) * 6, B, rng.normal(size=(B, arch.latent_dim)).astype(np.float32), k < 3))
    return out


# --------------------------------------------------------------------------------------------------------------------
# one step from a given state
# --------------------------------------------------------------------------------------------------------------------
def evaluate(arch, p, x, y, eps, train_decoder=True, bf16=False, training=True, grads=True, dtype=np.float64):
    """(cache, scalars, gradients) of one evaluation at parameters p.  bf16: with the bf16 engine's roundings (a batch below
    64 stamps: the unfused backward)."""
    fwd = vb if bf16 else vo
    pd = {k: np.asarray(v, dtype) for k, v in p.items()}
    xd, yd, ed = np.asarray(x, dtype), np.asarray(y, dtype), np.asarray(eps, dtype)
    c = fwd.forward(arch, pd, xd, ed, training=training)
    s = vo.losses(arch, c, yd)
    s.pop("nll")
    g = None
    if grads:
        if bf16:
            B = xd.shape[0]
            g = vb.backward(arch, pd, c, yd, train_decoder=train_decoder, fused=((B + 15) // 16 * 16) % 64 == 0)
        else:
            g = vo.backward(arch, pd, c, yd, train_decoder=train_decoder)
    return c, s, g


def adam_from(p, m, v, t, g, lr):
    """Legacy Adam (vo.adam_step) from the slots m, v and the counter t, on the tensors g names.  Returns copies
    (parameters, m, v, counter)."""
    st = vo.AdamState(lr=lr, t=int(t), m={k: np.array(m[k], dtype=np.float64) for k in g},
                      v={k: np.array(v[k], dtype=np.float64) for k in g})
    p2 = {k: np.array(a, dtype=np.float64) for k, a in p.items()}
    vo.adam_step(st, p2, {k: np.asarray(a, np.float64) for k, a in g.items()})
    return p2, st.m, st.v, st.t


def moving_after(arch, p, c):
    """The input BatchNorm's moving statistics after a training step whose batch statistics are in c."""
    q = {k: np.array(p[k], dtype=np.float64) for k in ("enc/bn/moving_mean", "enc/bn/moving_variance")}
    vo.bn_moving_update(arch, q, c)
    return q["enc/bn/moving_mean"], q["enc/bn/moving_variance"]


def single_step(arch, p, st, x, y, eps, train_decoder=True):
    """vo.train_step composed of the pieces above (p and st are updated in place); tests/test_trajectory_host.py holds the
    two against each other."""
    c, s, g = evaluate(arch, p, x, y, eps, train_decoder, dtype=p["enc/bn/gamma"].dtype)
    for k in g:
        st.m.setdefault(k, np.zeros_like(p[k]))
        st.v.setdefault(k, np.zeros_like(p[k]))
    p2, m2, v2, t2 = adam_from(p, st.m, st.v, st.t, g, st.lr)
    mean, var = moving_after(arch, p, c)
    p.update({k: p2[k] for k in g})
    p["enc/bn/moving_mean"], p["enc/bn/moving_variance"] = mean, var
    st.m.update(m2)
    st.v.update(v2)
    st.t = t2
    return s, g


# --------------------------------------------------------------------------------------------------------------------
# what a stale derived copy would cost
# --------------------------------------------------------------------------------------------------------------------
def groups(arch):
    """The groups of tensors the engine keeps a derived copy of: the folded first kernel, the padded encoder Dense, decoder
    Dense 0 and head tensors, and every conv / transposed-conv kernel alone (transformed, cast or re-laid per update)."""
    n2 = 2 * len(arch.filters)
    out = {"fold{enc/conv0/kernel,gamma,beta}": ["enc/conv0/kernel", "enc/bn/gamma", "enc/bn/beta"],
           "enc/dense/*": ["enc/dense/kernel", "enc/dense/bias"],
           "dec/dense0/*": ["dec/dense0/kernel", "dec/dense0/bias"],
           "dec/head/*": ["dec/head/kernel", "dec/head/bias"]}
    for j in range(1, n2):
        out[f"enc/conv{j}/kernel"] = [f"enc/conv{j}/kernel"]
    for j in range(n2):
        out[f"dec/convt{j}/kernel"] = [f"dec/convt{j}/kernel"]
    return out


def stale_effects(arch, p_prev, p_now, x, eps, bf16=False):
    """Per group that changed between p_prev and p_now: max over the outputs t and loc of |output with the group held at
    p_prev - output at p_now| / max|output at p_now| (training-mode forward on x, eps)."""
    fwd = vb if bf16 else vo
    x64, e64 = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    right = fwd.forward(arch, p_now, x64, e64, training=True)
    out = {}
    for name, members in groups(arch).items():
        if all(np.array_equal(p_prev[k], p_now[k]) for k in members):
            continue                                            # frozen in this step: nothing that could be stale
        q = dict(p_now)
        q.update({k: p_prev[k] for k in members})
        c = fwd.forward(arch, q, x64, e64, training=True)
        out[name] = max(relmax(c["t"], right["t"]), relmax(c["loc"], right["loc"]))
    return out


def teacher_trajectory(arch, p0, x, y, sched, lr, bf16=False):
    """The oracle's own run of the teacher schedule (optimizer state fresh at each change of stage): the parameters BEFORE
    every step, and after the last."""
    p = {k: v.copy() for k, v in p0.items()}
    states, st, stage = [], None, None
    for first, B, eps, dec in sched:
        if dec != stage:
            st, stage = vo.AdamState(lr=lr), dec
        states.append({k: v.copy() for k, v in p.items()})
        sl = slice(first, first + B)
        c, _, g = evaluate(arch, p, x[sl], y[sl], eps, dec, bf16=bf16)
        for k in g:
            st.m.setdefault(k, np.zeros_like(p[k]))
            st.v.setdefault(k, np.zeros_like(p[k]))
        p2, st.m, st.v, st.t = adam_from(p, st.m, st.v, st.t, g, lr)
        mean, var = moving_after(arch, p, c)
        p = p2
        p["enc/bn/moving_mean"], p["enc/bn/moving_variance"] = mean, var
    states.append(p)
    return states


def premise_table(arch, states, x, sched, bound, bf16=False):
    """rows (step k >= 2, group, effect, effect / bound) of stale_effects along a trajectory of states (the parameters before
    each step): what the comparison of step k's outputs at `bound` would see of a copy left at step k - 1's values."""
    rows = []
    for k in range(1, len(sched)):
        first, B, eps, _ = sched[k]
        eff = stale_effects(arch, states[k - 1], states[k], x[first:first + B], eps, bf16)
        rows += [(k + 1, name, e, e / bound) for name, e in eff.items()]
    return rows


def format_premise(title, rows, need=5.0):
    lines = [f"{title}: smallest effect of a one-step-stale group on t / loc, in units of the comparison's bound (needed {need:g})"]
    for name in dict.fromkeys(r[1] for r in rows):
        mine = [r for r in rows if r[1] == name]
        w = min(mine, key=lambda r: r[3])
        lines.append(f"    {name:36s} step {w[0]}: {w[2]:.3e} * max = {w[3]:7.1f} x bound{'' if w[3] >= need else '   <-- below'}")
    return "\n".join(lines)


# --------------------------------------------------------------------------------------------------------------------
# free-running trajectories
# --------------------------------------------------------------------------------------------------------------------
def queued_rows(first, B, n, steps):
    """first rows of dv_train_steps' batches: (first + k B) mod (n - B + 1)"""
    return [(first + k * B) % (n - B + 1) for k in range(steps)]


def run_steps(arch, p0, x, y, first, B, steps, seed, lr, dtype=np.float64):
    """The queued trajectory: `steps` train steps on rows queued_rows(...), eps of step k from the engine's generator with
    seed + k.  Returns (scalars per step, final parameters)."""
    p = {k: np.asarray(v, dtype).copy() for k, v in p0.items()}
    st = vo.AdamState(lr=lr)
    out = []
    for k, r0 in enumerate(queued_rows(first, B, x.shape[0], steps)):
        eps = vo.philox_normal(seed + k, 0, B, arch.latent_dim).astype(dtype)
        s, _ = vo.train_step(arch, p, st, np.asarray(x[r0:r0 + B], dtype), np.asarray(y[r0:r0 + B], dtype), eps)
        out.append({k2: float(v) for k2, v in s.items()})
    return out, p


def eval_scalars(arch, p, x, y, seed, dtype=np.float64, mse_sample=False):
    """One evaluation in inference mode (moving statistics) with the generator's eps for `seed`."""
    B = x.shape[0]
    eps = vo.philox_normal(seed, 0, B, arch.latent_dim).astype(dtype)
    c, s, _ = evaluate(arch, p, x, y, eps, training=False, grads=False, dtype=dtype)
    if mse_sample:
        s["mse"] = sample_mse(c, np.asarray(y, dtype), seed)
    return {k: float(v) for k, v in s.items()}


def sample_mse(c, y, seed):
    """Keras' "mse" on the model output, a SAMPLE of Normal(loc, scale) (model.py:158), drawn from the engine's generator"""
    e = vo.philox_normal(seed, MSE_STREAM, y.shape[0], int(np.prod(y.shape[1:]))).reshape(y.shape).astype(y.dtype)
    return ((y - (c["loc"] + c["scale"] * e)) ** 2).mean()


def fit_loop(n, nv, batch_size, epochs, shuffle_seed, seed0, train_fn, eval_fn, shuffle=True):
    """Keras Model.fit's bookkeeping for in-memory arrays.  Every epoch draws one permutation of the n rows from ONE generator
    seeded with shuffle_seed and walks it in batches of batch_size, the last one as small as it comes; every step - training,
    then validation, epoch after epoch - takes the next noise seed seed0 + 1, seed0 + 2, ...; an epoch's log is the mean of the
    per-batch values WEIGHTED BY THE BATCH SIZE; validation walks its rows in order, after the epoch's updates.
    train_fn(rows, seed) / eval_fn(rows, seed) -> dict of per-batch values.  Returns the history (val_* included)."""
    rng = np.random.default_rng(shuffle_seed)
    seed, hist = seed0, {}
    for _ in range(epochs):
        order = rng.permutation(n) if shuffle else np.arange(n)
        for prefix, rows_of, fn in (("", [order[b:b + batch_size] for b in range(0, n, batch_size)], train_fn),
                                    ("val_", [np.arange(b, min(b + batch_size, nv)) for b in range(0, nv, batch_size)], eval_fn)):
            tot, seen = {}, 0
            for rows in rows_of:
                seed += 1
                for k, v in fn(rows, seed).items():
                    tot[k] = tot.get(k, 0.0) + float(v) * len(rows)
                seen += len(rows)
            for k, v in tot.items():
                hist.setdefault(prefix + k, []).append(v / seen)
    return hist


def vae_fit(arch, p0, x, y, xv, yv, batch_size, epochs, shuffle_seed, seed0, lr, dtype=np.float64):
    """fit(x, y, validation_data=(xv, yv)) of the net compiled with metrics=["mse", kl_metric]: fit_loop over the oracle's
    train step and its inference-mode evaluation.  Returns (history, iterations)."""
    p = {k: np.asarray(v, dtype).copy() for k, v in p0.items()}
    st = vo.AdamState(lr=lr)
    x, y, xv, yv = (np.asarray(a, dtype) for a in (x, y, xv, yv))

    def metrics(c, s, yb, seed):
        return {"loss": s["loss"], "mse": sample_mse(c, yb, seed), "kl_metric": s["kl_reg"]}

    def train_fn(rows, seed):
        eps = vo.philox_normal(seed, 0, len(rows), arch.latent_dim).astype(dtype)
        c = vo.forward(arch, p, x[rows], eps, training=True)
        s = vo.losses(arch, c, y[rows])
        vo.adam_step(st, p, vo.backward(arch, p, c, y[rows]))
        vo.bn_moving_update(arch, p, c)
        return metrics(c, s, y[rows], seed)

    def eval_fn(rows, seed):
        eps = vo.philox_normal(seed, 0, len(rows), arch.latent_dim).astype(dtype)
        c = vo.forward(arch, p, xv[rows], eps, training=False)
        return metrics(c, vo.losses(arch, c, yv[rows]), yv[rows], seed)

    return fit_loop(x.shape[0], xv.shape[0], batch_size, epochs, shuffle_seed, seed0, train_fn, eval_fn), st.t


def free_bound(d32):
    """Bound of a free-running comparison, per number: the project's ELBO bound 1e-4, or 1.5 x the distance of the numpy
    float32 run of the same trajectory from float64 where that is larger, never above 1e-3."""
    return min(max(1e-4, 1.5 * d32), 1e-3)


def rel(a, b):
    return abs(a - b) / (abs(b) + 1e-30)
