"""CPU tests of tests/trajectory_oracle.py and of the premises tests/test_gpu_trajectory.py rests on: the helper's step is the
oracle's step, its fit loop is Keras' bookkeeping, a one-step-stale derived copy is visible at the bounds the teacher-forced
comparison uses, and a numpy float32 run of the free-running trajectories stays far enough inside their bound.  Run with -s
for the premise tables and the float32 distances."""
import numpy as np
import pytest

from oracle import vae_oracle as vo
from tests import trajectory_oracle as to

TEACHER, TEACHER_SEED, NEED, FREE_LR, QUEUE, FIT = to.TEACHER, to.TEACHER_SEED, to.NEED, to.FREE_LR, to.QUEUE, to.FIT


def _teacher_rows(net, kind):
    cfg = TEACHER[kind]
    arch = to.nets()[net]
    p, x, y = to.case(arch, 24, TEACHER_SEED, cfg["sigma_bias"])
    sched = to.teacher_schedule(arch, TEACHER_SEED + 1)
    states = to.teacher_trajectory(arch, p, x, y, sched, cfg["lr"], cfg["bf16"])
    return to.premise_table(arch, states, x, sched, cfg["bound"], cfg["bf16"])


def test_single_step_of_the_helper_is_the_oracles_train_step():
    arch = to.nets()["T8"]
    p, x, y = to.case(arch, 6, 3)
    eps = np.random.default_rng(5).normal(size=(6, arch.latent_dim))
    for dec in (True, False):
        pa, pb = ({k: v.copy() for k, v in p.items()} for _ in range(2))
        sa, sb = vo.AdamState(lr=1e-3), vo.AdamState(lr=1e-3)
        for _ in range(3):                      # slots that start non-zero, t >= 2
            ra, ga = vo.train_step(arch, pa, sa, x.astype(np.float64), y.astype(np.float64), eps, train_decoder=dec)
            rb, gb = to.single_step(arch, pb, sb, x, y, eps, train_decoder=dec)
            assert sa.t == sb.t and set(ga) == set(gb)
            for k in to.SCALARS:
                assert ra[k] == rb[k]
            for k in pa:
                np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
            for k in ga:
                np.testing.assert_array_equal(sa.m[k], sb.m[k], err_msg=k)
                np.testing.assert_array_equal(sa.v[k], sb.v[k], err_msg=k)
    # frozen decoder: nothing of it moved
    for k in p:
        if k.startswith("dec/"):
            np.testing.assert_array_equal(pb[k], p[k])


def test_fit_loop_gives_the_keras_weighted_means_on_a_hand_computable_case():
    """constant per-batch losses 1, 2, 3 with batch sizes 5, 5, 2: the epoch's loss is (5 + 10 + 6) / 12 = 1.75, not 2; the
    seeds run on through training and validation; one permutation per epoch from one generator."""
    seen = []

    def train_fn(rows, seed):
        seen.append(("t", seed, tuple(rows)))
        return {"loss": float((sum(s[0] == "t" for s in seen) - 1) % 3 + 1)}          # 1, 2, 3 in every epoch

    def eval_fn(rows, seed):
        seen.append(("v", seed, tuple(rows)))
        return {"loss": 10.0 if len(rows) == 5 else 20.0}

    h = to.fit_loop(12, 7, 5, 2, shuffle_seed=3, seed0=100, train_fn=train_fn, eval_fn=eval_fn)
    assert h["loss"] == [1.75, 1.75]
    assert h["val_loss"] == [(5 * 10.0 + 2 * 20.0) / 7] * 2
    assert [s[1] for s in seen] == list(range(101, 111))                                 # ten steps, ten consecutive seeds
    assert [s[0] for s in seen] == ["t", "t", "t", "v", "v"] * 2
    assert [len(s[2]) for s in seen] == [5, 5, 2, 5, 2] * 2
    rng = np.random.default_rng(3)
    for e in range(2):
        perm = rng.permutation(12)
        assert np.concatenate([s[2] for s in seen[5 * e:5 * e + 3]]).tolist() == perm.tolist()
        assert seen[5 * e + 3][2] == (0, 1, 2, 3, 4) and seen[5 * e + 4][2] == (5, 6)
    h = to.fit_loop(12, 0, 5, 1, 3, 0, lambda rows, seed: {"loss": 1.0}, None, shuffle=False)
    assert h == {"loss": [1.0]}


@pytest.mark.parametrize("net", ["T8", "T32"])
def test_a_stale_group_is_visible_to_the_fp32_comparison(net):
    """fp32, lr = 1e-3: along the oracle's own trajectory of the teacher schedule every group the engine keeps a derived copy
    of, held at its step k - 1 value, moves t or loc by at least 5 x the 2e-4 * max the outputs are compared at (k >= 2)."""
    rows = _teacher_rows(net, "fp32")
    print("\n" + to.format_premise(f"{net} fp32 lr 1e-3", rows, NEED))
    assert {r[1] for r in rows} == set(to.groups(to.nets()[net]))            # every group was looked at
    assert not [r for r in rows if r[3] < NEED]


def test_what_the_bf16_comparison_sees_of_a_stale_group():
    """bf16, lr = 1e-2, outputs compared at 1e-2 * max against the bf16-rounding oracle: every group but decoder Dense 0 and the
    folded first kernel meets the premise; those two are left to the bit-exact continuation test (part 2), which sees every
    group without a tolerance."""
    rows = _teacher_rows("T32", "bf16")
    print("\n" + to.format_premise("T32 bf16 lr 1e-2", rows, NEED))
    low = {r[1] for r in rows if r[3] < NEED}
    print("    left to the bit-exact continuation test:", sorted(low) or "none")
    assert low <= {"dec/dense0/*", "fold{enc/conv0/kernel,gamma,beta}"}, low


@pytest.mark.parametrize("net", ["T8", "T32"])
def test_float32_floor_of_the_free_running_comparisons(net):
    """The free-running comparisons (six queued steps; fit() over two epochs) at lr = 1e-4: the numpy float32 run of the same
    trajectory must stay below the cap of the bound (1e-3 / 1.5) in every number - else another seed is chosen here, on the
    CPU; the cap does not move."""
    arch = to.nets()[net]
    q = QUEUE
    p, x, y = to.case(arch, q["n"] + 6, q["seed"])
    r64, p64 = to.run_steps(arch, p, x[:q["n"]], y[:q["n"]], q["first"], q["B"], q["steps"], q["run_seed"], FREE_LR)
    r32, p32 = to.run_steps(arch, p, x[:q["n"]], y[:q["n"]], q["first"], q["B"], q["steps"], q["run_seed"], FREE_LR, np.float32)
    worst = max(to.rel(r32[k][s], r64[k][s]) for k in range(q["steps"]) for s in to.SCALARS)
    e64 = to.eval_scalars(arch, p64, x[q["n"]:], y[q["n"]:], q["eval_seed"])
    e32 = to.eval_scalars(arch, p32, x[q["n"]:], y[q["n"]:], q["eval_seed"], np.float32)
    worst_e = max(to.rel(e32[s], e64[s]) for s in to.SCALARS)
    f = FIT
    p, x, y = to.case(arch, f["n"] + f["nv"], f["seed"])
    args = (arch, p, x[:f["n"]], y[:f["n"]], x[f["n"]:], y[f["n"]:], f["batch_size"], f["epochs"], f["shuffle_seed"], f["seed0"], FREE_LR)
    h64, it = to.vae_fit(*args)
    h32, _ = to.vae_fit(*args, dtype=np.float32)
    assert it == 6 and sorted(h64) == ["kl_metric", "loss", "mse", "val_kl_metric", "val_loss", "val_mse"]
    worst_f = max(to.rel(h32[k][e], h64[k][e]) for k in h64 for e in range(2))
    print(f"\n{net}: numpy float32 run vs float64, relative: queued steps {worst:.2e}, eval afterwards {worst_e:.2e}, "
          f"fit history {worst_f:.2e}  (plain bound 1e-4; cap 1e-3)")
    assert max(worst, worst_e, worst_f) <= 1e-3 / 1.5
