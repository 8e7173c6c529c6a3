#!/usr/bin/env python3
"""SHA-256 of everything the posterior-path family returns, through the package: one line per result.  Two
trees - library and Python layer - compute the same bits exactly when the two outputs are equal:
    python tools/paths_bits.py > new.txt;  (cd /path/to/other/tree && python tools/paths_bits.py) > old.txt
    python tools/paths_bits.py --compare old.txt new.txt
Every case of tests/golden/paths_ref.npz, axis_paths_ref.npz and sparse_paths_ref.npz (sparse models with rows and without),
the models and path sets built as the tests build them (their `case` functions; device buffers start out as NaN as there, so
the padding columns of a model-major `coef` are digested too): `coef`, `paths(Xq)`, `step(Xs)`, `rollout` - for a batch with
the input scaler and without - then `SimpleQuadrotorGP.sample_rollouts` and `PreTrainedGP.sample_rollouts` on the models of
their tests."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from serving_bits import compare, digest  # noqa: E402

OUT = sys.stdout


def line(tag, a):
    print(tag, digest(a), file=OUT)


def path_set(tag, c, paths, rollouts):
    line(f"{tag} coef", paths.coef.cpu().numpy())
    line(f"{tag} paths(Xq)", paths(c["Xq"]))
    line(f"{tag} step(Xs)", paths.step(c["Xs"]))
    for what, traj in rollouts:
        line(f"{tag} rollout{what}", traj())


def batch_rollouts(mod, c, paths):
    return (("", lambda: mod.roll(paths, c)), (" without the input scaler", lambda: mod.roll(paths, c, in_scaler=None)))


def sampled(tag, out):
    assert not (out[0] == out[1]).all(), tag + ": the nominal trajectory came back (the sampling failed)"
    line(tag, out)


def run():
    import test_gpu_axis_paths as A
    import test_gpu_paths as E
    import test_gpu_sparse_paths as S
    from unmanned_aerial_vehicles_amd import PreTrainedGP, SimpleQuadrotorGP
    for name in E.CASE_NAMES:
        c, _, paths, _ = E.case(name)
        path_set(f"exact {name}", c, paths, (("", lambda: paths.rollout(c["x0"], c["U"], c["lin"])),))
    for name in A.CASE_NAMES:
        c, _, paths, _ = A.case(name)
        path_set(f"axis {name}", c, paths, batch_rollouts(A, c, paths) if name in A.ROLLOUT_CASES else ())
    for name in S.SINGLE:
        c, _, paths, _ = S.case(name)
        path_set(f"sparse {name} rows={len(c['X'])}", c, paths, (("", lambda: paths.rollout(c["x0"], c["U"], c["lin"])),))
    for name in S.BATCH:
        c, _, paths, _ = S.case(name)
        path_set(f"sparse batch {name} rows={len(c['X'])}", c, paths, batch_rollouts(S, c, paths) if name in S.ROLLOUT_BATCH else ())
    how = dict(n_rollouts=5, n_features=32, random_state=7)
    c, gp, _, _ = E.case("csv")
    sq = SimpleQuadrotorGP()
    sq.gp_model, sq.is_trained = gp, True
    sampled("SimpleQuadrotorGP.sample_rollouts", sq.sample_rollouts(c["x0"][0], c["U"].T, 0.02, **how))
    c, bg, _, _ = A.case("csv")
    pg = PreTrainedGP("/nonexistent/model.pkl")
    for keep in (list(range(6)), [0, 2, 3, 4, 5]):
        assert pg.load_dict(A.trainer_dict(c, bg, keep))
        sampled(f"PreTrainedGP.sample_rollouts models {keep}", pg.sample_rollouts(c["x0"][0], c["U"].T, 0.02, **how))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    with contextlib.redirect_stdout(sys.stderr):      # (what the models print while they load goes to stderr)
        run()
