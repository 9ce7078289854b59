"""Training beyond the first step, anchored to the oracle (tests/trajectory_oracle.py over oracle/vae_oracle.py).

The single-step parity tests (test_gpu_parity.py, test_gpu_bf16.py) stop after one update from fresh Adam slots.  Here the state
that changes from step to step - Adam at t >= 2 with slots that start non-zero, the trainable sets of both stages, the fresh
state of stage 2, the moving statistics of the input BatchNorm, and every tensor the engine derives from the parameters and
re-makes after an update (folded first kernel, padded Dense / head tensors, Winograd transforms, bf16 casts) - is compared
  1. step by step against the oracle started from the engine's own state (teacher-forced: nothing cascades, a failing step
     and tensor are named), at learning rates at which a one-step-stale derived copy moves the outputs by >= 5 bounds;
  2. bit for bit against a fresh engine given the trained state, which derives every copy from the parameters anew;
  3. free-running against the float64 oracle: six queued steps and fit() over two epochs, with the distance of a numpy
     float32 run of the same trajectory as the measured floor of the bound.
Bounds (none looser than the single-step tests'): outputs t, z, kl, loc, scale 2e-4 * max and the four scalars 1e-4 relative
(bf16, against the bf16-rounding oracle: 1e-2 * max, 5e-4); gradients 1e-3 * max, 2e-3 for d(gamma) / d(beta) (bf16: 5e-2);
parameters after the update 1e-2 * lr absolute against the oracle's Adam fed with the engine's gradients and started from the
engine's slots; slots rtol 5e-5, with an absolute floor of one float32 ulp of the update's operands (below); the step counter
exact; moving statistics 1e-6 absolute (bf16: rtol 1e-5 against the float64 statistics of the float32 input); eval_step on a
batch not trained on 1e-4 (bf16 2e-3); free-running numbers max(1e-4, 1.5 x the float32 run's distance), capped at 1e-3.

The slots' absolute floor.  m' = m + (g - m)(1 - b1) in float32 carries a rounding of each operand: up to 2^-24 of |g - m| and
of |m|, whatever m' comes to.  From t = 2 on 0.9 m and 0.1 g cancel in some of a tensor's 10^5 elements, and a relative bound
on m' alone fails there for ANY float32 evaluation (numpy float32 on the oracle's trajectory: 0.14 relative on one element of
dec/dense1/kernel at step 2, 2e-3 at step 3; 1.3e-5 at t = 1, where nothing cancels; the engine on an MI355X: 0.16 on one
element, printed with every run as "slot, relative error alone").  So: |m' - ref| <= 5e-5 |ref| +
2^-23 (|m| + |g|), and the same for v with g^2 - two ulps of the operands, seven decades below what a wrong slot, counter or
beta would change."""
import numpy as np
import pytest

from tests import margins
from tests import trajectory_oracle as to
from tests.test_gpu_parity import _grad_tol, _relmax

pytestmark = pytest.mark.gpu

ULP2 = 2.0 ** -23
MOVING = ("enc/bn/moving_mean", "enc/bn/moving_variance")


def _engine(arch, max_batch, bf16=False):
    from debvader_amd import engine as E

    return E.Engine(E.make_config(arch.input_shape, arch.latent_dim, tuple(arch.filters), tuple(arch.kernels),
                                  max_batch=max_batch, dtype=1 if bf16 else 0))


def _state(eng):
    """(parameters, m, v, iterations) as the engine holds them (float32)"""
    P = {n: eng.get_param(n) for n, _, _ in eng.specs}
    M = {n: eng.get_slot(n, 0) for n, _, tr in eng.specs if tr}
    V = {n: eng.get_slot(n, 1) for n, _, tr in eng.specs if tr}
    return P, M, V, eng.iterations


def _f64(d):
    return {k: v.astype(np.float64) for k, v in d.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_bit_equal(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], dict):
            _assert_bit_equal(a[k], b[k], f"{what} / {k}")
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


class _Worst:
    """the largest fraction of its bound that any comparison of a test used, per kind of comparison"""

    def __init__(self):
        self.rows = {}

    def add(self, kind, what, err, bound):
        frac = err / bound
        if kind not in self.rows or frac > self.rows[kind][1] / self.rows[kind][2]:
            self.rows[kind] = (what, err, bound)
        return frac <= 1.0

    def report(self, title):
        print(f"\n{title}: worst fraction of each bound")
        for kind, (what, err, bound) in self.rows.items():
            print(f"    {kind:34s} {err / bound:6.3f}  ({err:.3e} of {bound:.1e}: {what})")
        margins.record(title, [(f"{kind}"[:34], err, None, bound, what) for kind, (what, err, bound) in self.rows.items()],
                       "the worst case of each kind of comparison; engine = measured error")


# ----------------------------------------------------------------------------------------------------------------------
# 1. teacher-forced steps
# ----------------------------------------------------------------------------------------------------------------------
def _teacher(net, kind):
    cfg = to.TEACHER[kind]
    lr, bf16, tol_out = cfg["lr"], cfg["bf16"], cfg["bound"]
    tol_scal = 5e-4 if bf16 else 1e-4
    arch = to.nets()[net]
    p, x, y = to.case(arch, 24, to.TEACHER_SEED, cfg["sigma_bias"])
    sched = to.teacher_schedule(arch, to.TEACHER_SEED + 1)
    eps_eval = np.random.default_rng(to.TEACHER_SEED + 2).normal(size=(6, arch.latent_dim)).astype(np.float32)
    xe, ye = x[18:], y[18:]                       # never trained on
    eng = _engine(arch, 6, bf16)
    eng.set_params(p)
    eng.set_trainable(True, True)
    eng.optimizer_reset(lr)
    eng.upload(0, x[:18], y[:18])
    eng.upload(1, xe, ye)
    eng.keep_outputs(True)
    H, W, C = arch.input_shape
    trainable = [n for n, _, tr in eng.specs if tr]
    worst, failed, states, frozen = _Worst(), [], [], None

    def check(kind_, what, err, bound):
        if not worst.add(kind_, what, err, bound):
            failed.append((what, err, bound))

    for k, (first, B, eps, dec) in enumerate(sched):
        step = f"step {k + 1}"
        if k == 3:                                 # stage 2 of train_deblender: decoder frozen, a fresh optimizer
            eng.set_trainable(True, False)
            eng.optimizer_reset(lr)
            assert eng.iterations == 0
            for n in trainable:
                assert not eng.get_slot(n, 0).any() and not eng.get_slot(n, 1).any(), ("slot not zero after the reset", n)
        P, M, V, it = _state(eng)
        assert it == (k if k < 3 else k - 3), (step, it)
        if k == 3:
            frozen = {n: (P[n], M[n], V[n]) for n in trainable if n.startswith("dec/")}
        p64 = _f64(P)
        states.append(p64)
        sl = slice(first, first + B)
        c, ref, g = to.evaluate(arch, p64, x[sl], y[sl], eps, dec, bf16)
        assert set(g) == {n for n in trainable if dec or not n.startswith("dec/")}

        # the forward pass and the gradients of this step, from the state the step starts from
        out = eng.grad_step(0, first=first, B=B, eps=eps)
        acts = {"t": (B, arch.params_size), "z": (B, arch.latent_dim), "kl": (B,), "loc": (B, H, W, C), "scale": (B, H, W, C)}
        for a, shape in acts.items():
            check("output", f"{step} {a}", _relmax(eng.activation(a, shape), c[a]), tol_out)
        for s in to.SCALARS:
            check("scalar of the step", f"{step} {s}", to.rel(out[s], ref[s]), tol_scal)
        gg = {n: eng.get_grad(n) for n in g}
        for n in g:
            check("gradient", f"{step} {n}", _relmax(gg[n], g[n]), 5e-2 if bf16 else _grad_tol(n))

        # the update: the oracle's Adam from the engine's slots and counter, fed with the engine's gradients
        p2, m2, v2, t2 = to.adam_from(p64, M, V, it, _f64(gg), lr)
        mean2, var2 = to.moving_after(arch, p64, c)
        out2 = eng.train_step(0, first=first, B=B, eps=eps)
        for s in to.SCALARS:
            check("scalar of the step", f"{step} train_step {s}", to.rel(out2[s], ref[s]), tol_scal)
        assert eng.iterations == t2 == it + 1, (step, eng.iterations)
        Pn, Mn, Vn, _ = _state(eng)
        for n in g:
            check("parameter after Adam", f"{step} {n}", float(np.abs(Pn[n] - p2[n]).max()), 1e-2 * lr)
            g64 = gg[n].astype(np.float64)
            for name, got, want, ops in (("m", Mn[n], m2[n], np.abs(M[n]) + np.abs(g64)), ("v", Vn[n], v2[n], V[n] + g64 * g64)):
                excess = np.abs(got - want) / (5e-5 * np.abs(want) + ULP2 * ops + 1e-30)
                check("Adam slot (fraction of its bound)", f"{step} {name} {n}", float(excess.max()), 1.0)
                nz = np.abs(want) > 1e-30            # (not asserted: what a relative bound alone would have met)
                if nz.any():
                    worst.add("  [slot, relative error alone]", f"{step} {name} {n}",
                              float((np.abs(got - want)[nz] / np.abs(want)[nz]).max()), 5e-5)
        if not dec:
            for n, (fp, fm, fv) in frozen.items():           # frozen decoder: no bit of it or of its slots moves
                assert np.array_equal(_bits(Pn[n]), _bits(fp)), (step, n)
                assert np.array_equal(_bits(Mn[n]), _bits(fm)) and np.array_equal(_bits(Vn[n]), _bits(fv)), (step, n)
        for n, want in zip(MOVING, (mean2, var2)):
            if bf16:     # (updated from the prefetched statistics of the float32 input)
                check("moving statistic", f"{step} {n}", float((np.abs(Pn[n] - want) / np.abs(want)).max()), 1e-5)
            else:
                check("moving statistic", f"{step} {n}", float(np.abs(Pn[n] - want).max()), 1e-6)

        if k in (2, 4):                             # inference mode, with the moving statistics that have moved
            oe = eng.eval_step(1, first=0, B=6, eps=eps_eval)
            _, re_, _ = to.evaluate(arch, _f64(Pn), xe, ye, eps_eval, bf16=bf16, training=False, grads=False)
            for s in to.SCALARS:
                check("eval_step after training", f"after {step} {s}", abs(oe[s] - re_[s]),
                      2e-3 * abs(re_[s]) + 1e-6 if bf16 else 1e-4 * abs(re_[s]))
    states.append(_f64(_state(eng)[0]))
    eng.close()
    worst.report(f"teacher-forced steps, {net} {kind}, lr {lr:g}")
    assert not failed, failed

    # the power of the comparison on THIS trajectory: what a copy left one step stale would have moved
    rows = to.premise_table(arch, states, x, sched, tol_out, bf16)
    print(to.format_premise(f"{net} {kind} (the engine's trajectory)", rows, to.NEED))
    low = {r[1] for r in rows if r[3] < to.NEED}
    if bf16:
        print("    left to the bit-exact continuation test:", sorted(low) or "none")
        assert low <= {"dec/dense0/*", "fold{enc/conv0/kernel,gamma,beta}"}, low
    else:
        assert not low, low


@pytest.mark.parametrize("net,kind", [("T8", "fp32"), ("T32", "fp32"), ("T32", "bf16")])
def test_teacher_forced_steps_against_the_oracle(net, kind):
    """Five train steps (stage 1, then stage 2 with a fresh optimizer), each checked against one oracle step from the engine's
    own state: outputs, scalars, gradients, the Adam update at t >= 2, slots, counter, frozen tensors, moving statistics,
    eval_step after steps 3 and 5."""
    _teacher(net, kind)


# ----------------------------------------------------------------------------------------------------------------------
# 2. a fresh engine given the trained state continues bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def _snapshot(eng, grads=True):
    P, M, V, it = _state(eng)
    out = {"param": P, "m": M, "v": V, "iterations": it}
    if grads:
        out["grad"] = {n: eng.get_grad(n) for n in M}
    return out


def _clone(arch, src, bf16, lr, dec, data):
    """a fresh engine with src's parameters, slots and counter: every derived tensor is made from the parameters anew"""
    P, M, V, it = _state(src)
    eng = _engine(arch, src.max_batch, bf16)
    eng.set_params(P)
    eng.set_trainable(True, dec)
    eng.optimizer_reset(lr)
    for n in M:
        eng.set_slot(n, 0, M[n])
        eng.set_slot(n, 1, V[n])
    eng.iterations = it
    eng.upload(0, *data)
    eng.keep_outputs(True)
    return eng


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_fresh_engine_given_the_trained_state_continues_bit_for_bit(kind):
    """After three steps of stage 1, and again after a step of stage 2, a second engine is given the first one's parameters,
    slots and counter; the same next gradient step and train step on both must agree in every bit of every gradient,
    parameter, slot, moving statistic and scalar.  A fold, pad, Winograd transform or bf16 cast left stale in the trained
    engine is a bit difference here."""
    cfg = to.TEACHER[kind]
    lr, bf16 = cfg["lr"], cfg["bf16"]
    arch = to.nets()["T32"]
    p, x, y = to.case(arch, 18, to.TEACHER_SEED, cfg["sigma_bias"])
    sched = to.teacher_schedule(arch, to.TEACHER_SEED + 1)
    eng = _engine(arch, 6, bf16)
    eng.set_params(p)
    eng.set_trainable(True, True)
    eng.optimizer_reset(lr)
    eng.upload(0, x, y)
    eng.keep_outputs(True)

    def continue_both(dec, first, B, eps, what):
        twin = _clone(arch, eng, bf16, lr, dec, (x, y))
        _assert_bit_equal(_snapshot(eng, False), _snapshot(twin, False), f"{what}: the copied state")
        res = []
        for e in (eng, twin):
            og = e.grad_step(0, first=first, B=B, eps=eps)
            grads = {n: e.get_grad(n) for n, _, tr in e.specs if tr and (dec or not n.startswith("dec/"))}
            ot = e.train_step(0, first=first, B=B, eps=eps)
            res.append({"grad_step": og, "grads": grads, "train_step": ot, "after": _snapshot(e, False)})
        twin.close()
        _assert_bit_equal(res[0], res[1], what)
        assert res[0]["after"]["iterations"] >= 2

    for first, B, eps, _ in sched[:3]:
        eng.train_step(0, first=first, B=B, eps=eps)
    continue_both(True, *sched[3][:3], "stage 1 after three steps")
    eng.set_trainable(True, False)
    eng.optimizer_reset(lr)
    for first, B, eps, _ in sched[3:]:
        eng.train_step(0, first=first, B=B, eps=eps)
    continue_both(False, *sched[2][:3], "stage 2 after two steps")
    eng.close()


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_queued_steps_equal_single_steps_in_every_tensor(kind):
    """train_steps(slot, first, B, 4) - engine-drawn eps, seeds seed + k, rows (first + k B) mod (n - B + 1) - against the same
    four steps as single train_step calls on another engine: every parameter, both slots, the moving statistics, the counter
    and the scalars of the last step, bit for bit."""
    cfg = to.TEACHER[kind]
    arch = to.nets()["T32"]
    p, x, y = to.case(arch, 18, to.TEACHER_SEED, cfg["sigma_bias"])
    res = []
    for queued in (True, False):
        eng = _engine(arch, 6, cfg["bf16"])
        eng.set_params(p)
        eng.optimizer_reset(cfg["lr"])
        eng.upload(0, x, y)
        if queued:
            out = eng.train_steps(0, 2, 6, 4, seed=300)
        else:
            for k, r0 in enumerate(to.queued_rows(2, 6, 18, 4)):
                out = eng.train_step(0, first=r0, B=6, seed=300 + k)
        res.append({"last": out, "state": _snapshot(eng, False)})
        eng.close()
    assert res[0]["state"]["iterations"] == 4
    _assert_bit_equal(res[0], res[1], "queued vs single steps")


_ORDER_CHILD = r'''
import sys, zlib, numpy as np
sys.path.insert(0, %r)
from tests import test_gpu_trajectory as T
print("STATE", T._two_stage_state_crc(%r))
'''


def _two_stage_state_crc(kind):
    """CRC of every parameter, slot and the counter after four queued steps of stage 1 and two single steps of stage 2"""
    import zlib

    cfg = to.TEACHER[kind]
    arch = to.nets()["T32"]
    p, x, y = to.case(arch, 18, to.TEACHER_SEED, cfg["sigma_bias"])
    eng = _engine(arch, 6, cfg["bf16"])
    eng.set_params(p)
    eng.optimizer_reset(cfg["lr"])
    eng.upload(0, x, y)
    eng.train_steps(0, 2, 6, 4, seed=300)
    eng.set_trainable(True, False)
    eng.optimizer_reset(cfg["lr"])
    for k in range(2):
        eng.train_step(0, first=6 * k, B=6, seed=400 + k)
    P, M, V, it = _state(eng)
    eng.close()
    crc = it
    for d in (P, M, V):
        for n in sorted(d):
            crc = zlib.crc32(_bits(d[n]).tobytes(), crc)
    return crc


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_update_orders_without_early_adam_leave_the_same_state(kind):
    """The update of the other stream orders - DV_NO_EARLY_ADAM=1: every range updated at the end of the step, where the rule
    `opt_dec && adam_done_from > n_enc_train` decides about the padded decoder tensors; DV_NO_OVERLAP=1: one stream - must leave
    the state of the default order, which the tests above anchor to the oracle: every parameter, slot and the counter after
    four queued steps of stage 1 and two steps of stage 2, bit for bit.  (The switches are read once per process: children.)"""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    switches = ("DV_NO_EARLY_ADAM", "DV_NO_OVERLAP", "DV_FORCE_COMM")
    want = _two_stage_state_crc(kind)                          # this process: the default order
    for extra in ({"DV_NO_EARLY_ADAM": "1"}, {"DV_NO_OVERLAP": "1"}):
        env = {k: v for k, v in os.environ.items() if k not in switches}
        r = subprocess.run([sys.executable, "-c", _ORDER_CHILD % (root, kind)], env=dict(env, **extra),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("STATE ")][-1]
        assert got == f"STATE {want}", (extra, got, want)


# ----------------------------------------------------------------------------------------------------------------------
# 3. free-running against the float64 oracle
# ----------------------------------------------------------------------------------------------------------------------
def _free_rows(worst, rows, what, got, r64, r32):
    d_eng, d32 = to.rel(got, r64), to.rel(r32, r64)
    bound = to.free_bound(d32)
    rows.append((what, d_eng, d32, bound, "relative to the float64 run; other impl = the numpy float32 run"))
    return worst.add("free-running number", what, d_eng, bound)


@pytest.mark.parametrize("net", ["T8", "T32"])
def test_queued_trajectory_against_the_free_running_oracle(net):
    """Six queued steps at lr = 1e-4: the scalars of the last step and an eval_step afterwards on stamps not trained on, against
    the float64 oracle's own run of the six steps (eps from the restated generator)."""
    arch = to.nets()[net]
    q = to.QUEUE
    n = q["n"]
    p, x, y = to.case(arch, n + 6, q["seed"])
    run = (arch, p, x[:n], y[:n], q["first"], q["B"], q["steps"], q["run_seed"], to.FREE_LR)
    r64, p64 = to.run_steps(*run)
    r32, p32 = to.run_steps(*run, dtype=np.float32)
    e64 = to.eval_scalars(arch, p64, x[n:], y[n:], q["eval_seed"])
    e32 = to.eval_scalars(arch, p32, x[n:], y[n:], q["eval_seed"], np.float32)
    assert max(to.rel(r32[-1][s], r64[-1][s]) for s in to.SCALARS) <= 1e-3 / 1.5         # (tests/test_trajectory_host.py)
    eng = _engine(arch, q["B"])
    eng.set_params(p)
    eng.optimizer_reset(to.FREE_LR)
    eng.upload(0, x[:n], y[:n])
    eng.upload(1, x[n:], y[n:])
    out = eng.train_steps(0, q["first"], q["B"], q["steps"], seed=q["run_seed"])
    assert eng.iterations == q["steps"]
    oe = eng.eval_step(1, first=0, B=6, seed=q["eval_seed"])
    eng.close()
    worst, rows, ok = _Worst(), [], True
    for s in to.SCALARS:
        ok &= _free_rows(worst, rows, f"step 6 {s}", out[s], r64[-1][s], r32[-1][s])
        ok &= _free_rows(worst, rows, f"eval afterwards {s}", oe[s], e64[s], e32[s])
    margins.record(f"six queued steps vs the free-running float64 oracle, {net} fp32, lr 1e-4", rows)
    worst.report(f"six queued steps, free-running, {net}")
    assert ok, [r[:4] for r in rows if r[1] > r[3]]


@pytest.mark.parametrize("net", ["T8", "T32"])
def test_fit_history_against_the_free_running_oracle(net):
    """fit() over two epochs of 12 stamps in batches of 5 (three steps per epoch, the last of 2 stamps) with 7 validation
    stamps (batches of 5 and 2), metrics ["mse", kl_metric]: all twelve History numbers against the oracle's restatement of the
    loop - permutation stream, seed sequence, batch-size-weighted means, validation in inference mode after the epoch."""
    from debvader_amd.model import model
    from debvader_amd.training.metrics import vae_loss

    arch = to.nets()[net]
    f = to.FIT
    n = f["n"]
    p, x, y = to.case(arch, n + f["nv"], f["seed"])
    args = (arch, p, x[:n], y[:n], x[n:], y[n:], f["batch_size"], f["epochs"], f["shuffle_seed"], f["seed0"], to.FREE_LR)
    h64, it64 = to.vae_fit(*args)
    h32, _ = to.vae_fit(*args, dtype=np.float32)
    net_, _, _, _ = model.create_model_vae(arch.input_shape, arch.latent_dim, list(arch.filters), list(arch.kernels),
                                           max_batch=f["batch_size"], seed=7)
    net_._core.engine.set_params(p)
    net_._core.seed_counter = f["seed0"]

    def kl_metric(y_true, y_pred):
        return sum(net_.losses)

    net_.compile(optimizer=model.Adam(learning_rate=to.FREE_LR), loss=vae_loss, metrics=["mse", kl_metric])
    hist = net_.fit(x[:n], y[:n], epochs=f["epochs"], batch_size=f["batch_size"], shuffle=True, verbose=0,
                    shuffle_seed=f["shuffle_seed"], validation_data=(x[n:], y[n:]))
    assert net_._core.engine.iterations == it64 == 6
    assert net_._core.seed_counter == f["seed0"] + 10
    net_._core.engine.close()
    assert sorted(hist.history) == sorted(h64) == ["kl_metric", "loss", "mse", "val_kl_metric", "val_loss", "val_mse"]
    worst, rows, ok = _Worst(), [], True
    for k in sorted(h64):
        assert len(hist.history[k]) == 2
        for e in range(2):
            ok &= _free_rows(worst, rows, f"{k}[{e}]", hist.history[k][e], h64[k][e], h32[k][e])
    margins.record(f"fit() history vs the free-running float64 oracle, {net} fp32, lr 1e-4", rows)
    worst.report(f"fit() over two epochs, free-running, {net}")
    assert ok, [r[:4] for r in rows if r[1] > r[3]]
