"""Regenerate tests/golden/axis_cov_ref.npz: joint posterior covariances of the per-axis GP batch - six scalar ARD GPs on
shared inputs, each behind an input scaler and a target scaler (the layout of src/px4/gp_trainer.py:139-179 as
src/px4/pretrained_gp.py:52-98 serves it) - and Cholesky draws from them, in RAW units.  Needs NumPy, SciPy and scikit-learn
only.

    python tests/golden/make_golden_axis_cov.py [out.npz]

With z = (x - sx.mean_) / sx.scale_ the scaled query rows, Sigma_b model b's posterior covariance on them (WhiteKernel level on
the diagonal only, not clipped) and sy_b its target scaler: mean[:, b] = sy_b.mean_ + sy_b.scale_ mu_b(z), cov[..., b] =
sy_b.scale_^2 Sigma_b.

Cases (prefix_*):
  csv - the six models of make_golden_axis_jac.py::case_csv (X10 / Y6 of csv_170501.npz, one StandardScaler on X, per axis b a
        target scaler and C(1, fixed) * RBF(np.roll(np.linspace(0.6, 3.0, 10), b)) + WhiteKernel(0.02 (b + 1)), alpha 1e-6,
        optimizer=None).  csv_mean / csv_cov: scikit-learn's own predict(return_cov=True) per model on 25 rows - Xq10[:17]
        followed by the 8 training rows X10[q_train_idx[:8]], where the covariance is what is left of 1 after cancellation
        down to the noise level; csv_mean72 / csv_cov72: the same on the 64 Xq10 rows + those 8 training rows (the large
        route).  Hyper-parameters and scalers to rebuild the models.  csv_closed_vs_sk: the closed form below against
        scikit-learn's return_cov, per model, relative to the block's largest entry - the check that the closed form is right.
  ref - the reference trainer's own six models as frozen in trainer_ref.npz (N = 240); queries: its 8 Xq rows followed by
        X[:17].  The covariance from the stored L and theta in closed form: K(Z, Z) + noise I - V^T V, V = solve_triangular(L, K*^T).

Draws (*_draws, (25, 6, 8)): z = RandomState(0).standard_normal((6, 25, 8)), draws[:, b, :] = mean[:, b, None] +
cholesky(cov[..., b]) @ z[b].  The script stops unless every one of the twelve covariances factorises as it is, and unless a
1e-12 relative symmetric perturbation of a covariance moves its draws by less than 1e-10 of their scale (*_draw_shift: the
measured figures per model)."""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from scipy.linalg import solve_triangular  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["x_residual", "y_residual", "z_residual", "vx_residual", "vy_residual", "vz_residual"]
N_DRAWS = 8


def rbf(A, B, ls):
    d = A[:, None, :] / ls - B[None, :, :] / ls
    return np.exp(-0.5 * np.sum(d * d, axis=2))


def closed_form(Xt, alpha, L, ls, noise, Z):
    """One scalar model (sf2 = 1): mu (M,), Sigma (M, M) = K(Z, Z) + noise I - V^T V, symmetrised."""
    ks = rbf(Z, Xt, ls)                                   # (M, N)
    V = solve_triangular(L, ks.T, lower=True)             # (N, M)
    S = rbf(Z, Z, ls) + noise * np.eye(len(Z)) - V.T @ V
    return ks @ alpha, 0.5 * (S + S.T)


def draws(mean, cov, seed=0):
    """mean (M, B), cov (M, M, B) -> (M, B, N_DRAWS); every covariance must factorise as it is."""
    M, B = mean.shape
    z = np.random.RandomState(seed).standard_normal((B, M, N_DRAWS))
    out = np.empty((M, B, N_DRAWS))
    for b in range(B):
        out[:, b, :] = mean[:, b, None] + np.linalg.cholesky(cov[..., b]) @ z[b]       # raises LinAlgError: the script stops
    return out


def draw_shift(mean, cov):
    """Per model: how far a 1e-12 relative symmetric perturbation of the covariance moves the draws, relative to their scale."""
    base = draws(mean, cov)
    rng = np.random.RandomState(12345)
    M, B = mean.shape
    out = np.empty(B)
    for b in range(B):
        E = rng.uniform(-1.0, 1.0, (M, M))
        pert = cov.copy()
        pert[..., b] = cov[..., b] * (1.0 + 1e-12 * 0.5 * (E + E.T))
        moved = draws(mean, pert)
        scale = np.max(np.abs(base[:, b, :] - mean[:, b, None]))
        out[b] = np.max(np.abs(moved[:, b, :] - base[:, b, :])) / scale
    assert out.max() < 1e-10, out
    return out


def case_ref(out):
    tr = np.load(os.path.join(HERE, "trainer_ref.npz"))
    D = tr["X"].shape[1]
    Xq = np.vstack([tr["Xq"], tr["X"][:17]])
    mean, cov = np.empty((len(Xq), 6)), np.empty((len(Xq), len(Xq), 6))
    for b, n in enumerate(NAMES):
        th = tr[f"{n}_theta"]
        Z = (Xq - tr[f"{n}_sx_mean"]) / tr[f"{n}_sx_scale"]
        mu, S = closed_form(tr[f"{n}_X_train"], tr[f"{n}_alpha"], tr[f"{n}_L"], np.exp(th[:D]), float(np.exp(th[D])), Z)
        sy_mean, sy_scale = float(tr[f"{n}_sy_mean"][0]), float(tr[f"{n}_sy_scale"][0])
        mean[:, b], cov[..., b] = sy_mean + sy_scale * mu, sy_scale ** 2 * S
    out["ref_Xq"], out["ref_mean"], out["ref_cov"] = Xq, mean, cov
    out["ref_draws"] = draws(mean, cov)
    out["ref_draw_shift"] = draw_shift(mean, cov)


def case_csv(out):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from sklearn.preprocessing import StandardScaler
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    D, B = X.shape[1], Y.shape[1]
    Xtrain8 = X[d["q_train_idx"][:8]]
    Xq = np.vstack([d["Xq10"][:17], Xtrain8])
    Xq72 = np.vstack([d["Xq10"], Xtrain8])
    sx = StandardScaler().fit(X)
    Xs = sx.transform(X)
    ls_all, noise_all, sy_mean, sy_scale = [], [], [], []
    res = {25: (np.empty((25, B)), np.empty((25, 25, B))), 72: (np.empty((72, B)), np.empty((72, 72, B)))}
    chk = np.empty(B)
    for b in range(B):
        sy = StandardScaler().fit(Y[:, [b]])
        ls, noise = np.roll(np.linspace(0.6, 3.0, D), b), 0.02 * (b + 1)
        kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls) + WhiteKernel(noise)
        g = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=False, optimizer=None)
        g.fit(Xs, sy.transform(Y[:, [b]]).ravel())
        for Q, (mean, cov) in ((Xq, res[25]), (Xq72, res[72])):
            m, c = g.predict(sx.transform(Q), return_cov=True)
            mean[:, b] = sy.inverse_transform(m.reshape(-1, 1)).ravel()
            cov[..., b] = sy.scale_[0] ** 2 * c
        # the closed form (case ref's) against scikit-learn's own return_cov on the same model
        _, S = closed_form(g.X_train_, g.alpha_, g.L_, ls, noise, sx.transform(Xq))
        c25 = res[25][1][..., b]
        chk[b] = np.max(np.abs(sy.scale_[0] ** 2 * S - c25)) / np.max(np.abs(c25))
        ls_all.append(ls); noise_all.append(noise); sy_mean.append(float(sy.mean_[0])); sy_scale.append(float(sy.scale_[0]))
    out["csv_Xq"], out["csv_mean"], out["csv_cov"] = Xq, res[25][0], res[25][1]
    out["csv_Xq72"], out["csv_mean72"], out["csv_cov72"] = Xq72, res[72][0], res[72][1]
    out["csv_sx_mean"], out["csv_sx_scale"] = sx.mean_, sx.scale_
    out["csv_sy_mean"], out["csv_sy_scale"] = np.array(sy_mean), np.array(sy_scale)
    out["csv_ls"], out["csv_noise"] = np.stack(ls_all), np.array(noise_all)
    out["csv_closed_vs_sk"] = chk
    out["csv_draws"] = draws(res[25][0], res[25][1])
    out["csv_draw_shift"] = draw_shift(res[25][0], res[25][1])


def main(path):
    out = {}
    case_ref(out)
    case_csv(out)
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    out = main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "axis_cov_ref.npz"))
    for k, v in out.items():
        print(k, v.shape, v.ravel()[:3])
