"""Regenerate tests/golden/axis_jac_ref.npz: input gradients of the per-axis GP batch - six scalar ARD GPs on shared inputs,
each behind an input scaler and a target scaler (the layout of src/px4/gp_trainer.py:139-179 as src/px4/pretrained_gp.py:52-98
serves it) - in RAW units.  Needs NumPy, SciPy and scikit-learn only.

    python tests/golden/make_golden_axis_jac.py [out.npz]

With x a raw query row, z = (x - sx.mean_) / sx.scale_, mu_b / var_b model b's posterior on the scaled inputs (closed forms
of the RBF kernel in NumPy fp64, c = K^-1 k* by two solve_triangular calls with the model's own factor L) and sy_b its target
scaler:

    J[m, b, d]    = sy_b.scale_ / sx.scale_[d] * d mu_b / d z_d
    dstd[m, b, d] = |sy_b.scale_| / sx.scale_[d] * (d var_b / d z_d) / (2 sigma_b)            (0 where sigma_b = 0)
    dvar[m, b, d] = d var_b / d z_d                  (normalised-target units, scaled inputs: what the GPU kernels return)

Cases (prefix_*):
  ref - the reference trainer's own six models as frozen in trainer_ref.npz (theta, X_train, alpha, L, scalers per axis);
        queries: its 8 Xq rows followed by X[:17] (25 rows).  ref_pred = [mean, std] of the first 8 rows against the stored
        outputs of the reference's PreTrainedGP.predict_residual, relative to the largest entry.
  csv - X10 / Y6 of csv_170501.npz: one StandardScaler on X, per axis b a StandardScaler on the target and
        C(1.0, fixed) * RBF(np.roll(np.linspace(0.6, 3.0, 10), b)) + WhiteKernel(0.02 (b + 1)), alpha 1e-6, normalize_y=False,
        optimizer=None; queries: the 64 Xq10 rows followed by the 8 training rows X10[q_train_idx[:8]] (72 rows).  Also stores
        the scalers and hyper-parameters a test needs to rebuild the models; csv_pred = [mean, std] against scikit-learn's
        own predict through the scalers.

Every comparison of J, dstd and dvar is relative to the largest entry OF THE SAME INPUT COLUMN: the yaw-rate column of the
flight data has a standard deviation of 1e-21 and is scaled to unit variance like every other column (scikit-learn's
constant-feature rule), so raw Jacobian entries of that column are ~1e16 .. 1e21 and would swamp a max-norm.  *_chk = per-column
maxima [J, dstd, dvar] (3 x D) against the explicit inverse; *_fd = [J, d std^2 / dx = 2 std dstd] (2 x D), as jac_ref.npz
differences the mean and the variance, against fourth-order central differences of scikit-learn's own predict(return_std=True)
through the scalers, with the step 1e-3 * sx.scale_[d] for input d."""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from scipy.linalg import solve_triangular  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FD_H = 1e-3
NAMES = ["x_residual", "y_residual", "z_residual", "vx_residual", "vy_residual", "vz_residual"]


def colrel(a, b):
    """max |a - b| per input column (last axis), relative to the largest |b| of that column."""
    D = b.shape[-1]
    a, b = a.reshape(-1, D), b.reshape(-1, D)
    return np.max(np.abs(a - b), axis=0) / np.maximum(np.max(np.abs(b), axis=0), 1e-300)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def closed_form(Xt, alpha, L, ls, noise, Z, explicit_inverse=False):
    """One scalar model (sf2 = 1, no target normalisation) at scaled queries Z: mu (M,), var (M,) with the WhiteKernel level
    (clipped at 0 as scikit-learn clips it), dmu (M, D), dvar (M, D) - the gradient of the unclipped variance."""
    diff = Xt[None, :, :] - Z[:, None, :]                                      # (M, N, D): x_j - z
    k = np.exp(-0.5 * np.sum((diff / ls) ** 2, axis=2))                        # (M, N)
    u = diff / ls ** 2
    mu = k @ alpha
    dmu = np.einsum("mj,mjd,j->md", k, u, alpha)
    if explicit_inverse:
        Li = solve_triangular(L, np.eye(len(Xt)), lower=True)
        V = Li @ k.T
        c = Li.T @ V
    else:
        V = solve_triangular(L, k.T, lower=True)                               # (N, M)
        c = solve_triangular(L.T, V, lower=False)
    var = np.maximum(1.0 + noise - np.sum(V * V, axis=0), 0.0)
    dvar = -2.0 * np.einsum("mj,mjd,jm->md", k, u, c)
    return mu, var, dmu, dvar


def raw_units(mu, var, dmu, dvar, sx_scale, sy_mean, sy_scale):
    """The chain rule through the scalers: mean, std, J, dstd of one axis in raw units."""
    mean = mu * sy_scale + sy_mean
    sig = np.sqrt(var)
    std = np.abs(sig * sy_scale)
    J = sy_scale * dmu / sx_scale[None, :]
    g = np.zeros_like(dvar)
    pos = sig > 0.0
    g[pos] = dvar[pos] / (2.0 * sig[pos, None])
    dstd = abs(sy_scale) * g / sx_scale[None, :]
    return mean, std, J, dstd


def axis_case(models, Xq, explicit_inverse=False):
    """models: list of dicts (Xt, alpha, L, ls, noise, sx_mean, sx_scale, sy_mean, sy_scale) -> mean (M, B), std (M, B),
    J (M, B, D), dstd (M, B, D), dvar (M, B, D)."""
    cols = []
    for m in models:
        Z = (Xq - m["sx_mean"]) / m["sx_scale"]
        mu, var, dmu, dvar = closed_form(m["Xt"], m["alpha"], m["L"], m["ls"], m["noise"], Z, explicit_inverse)
        cols.append(raw_units(mu, var, dmu, dvar, m["sx_scale"], m["sy_mean"], m["sy_scale"]) + (dvar,))
    return tuple(np.stack([c[i] for c in cols], axis=1) for i in range(5))


def case_ref(out):
    tr = np.load(os.path.join(HERE, "trainer_ref.npz"))
    D = tr["X"].shape[1]
    models = []
    for n in NAMES:
        th = tr[f"{n}_theta"]
        models.append({"Xt": tr[f"{n}_X_train"], "alpha": tr[f"{n}_alpha"], "L": tr[f"{n}_L"], "ls": np.exp(th[:D]),
                       "noise": float(np.exp(th[D])), "sx_mean": tr[f"{n}_sx_mean"], "sx_scale": tr[f"{n}_sx_scale"],
                       "sy_mean": float(tr[f"{n}_sy_mean"][0]), "sy_scale": float(tr[f"{n}_sy_scale"][0])})
    Xq = np.vstack([tr["Xq"], tr["X"][:17]])
    mean, std, J, dstd, dvar = axis_case(models, Xq)
    _, _, J2, dstd2, dvar2 = axis_case(models, Xq, explicit_inverse=True)
    out["ref_Xq"], out["ref_mean"], out["ref_std"], out["ref_J"], out["ref_dstd"], out["ref_dvar"] = Xq, mean, std, J, dstd, dvar
    out["ref_pred"] = np.array([rel(mean[:8], tr["pred_mean"]), rel(std[:8], tr["pred_std"])])
    out["ref_chk"] = np.stack([colrel(J2, J), colrel(dstd2, dstd), colrel(dvar2, dvar)])


def case_csv(out):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from sklearn.preprocessing import StandardScaler
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    X, Y = d["X10"], d["Y6"]
    D, B = X.shape[1], Y.shape[1]
    Xq = np.vstack([d["Xq10"], X[d["q_train_idx"][:8]]])
    sx = StandardScaler().fit(X)
    Xs = sx.transform(X)
    models, gps, sys_ = [], [], []
    for b in range(B):
        sy = StandardScaler().fit(Y[:, [b]])
        ls, noise = np.roll(np.linspace(0.6, 3.0, D), b), 0.02 * (b + 1)
        kern = ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls) + WhiteKernel(noise)
        g = GaussianProcessRegressor(kernel=kern, alpha=1e-6, normalize_y=False, optimizer=None)
        g.fit(Xs, sy.transform(Y[:, [b]]).ravel())
        gps.append(g)
        sys_.append(sy)
        models.append({"Xt": g.X_train_, "alpha": g.alpha_, "L": g.L_, "ls": ls, "noise": noise, "sx_mean": sx.mean_,
                       "sx_scale": sx.scale_, "sy_mean": float(sy.mean_[0]), "sy_scale": float(sy.scale_[0])})
    mean, std, J, dstd, dvar = axis_case(models, Xq)
    _, _, J2, dstd2, dvar2 = axis_case(models, Xq, explicit_inverse=True)

    def sk_predict(Q):
        ms, ss = [], []
        for g, sy in zip(gps, sys_):
            m, s = g.predict(sx.transform(Q), return_std=True)
            ms.append(sy.inverse_transform(m.reshape(-1, 1)).ravel())
            ss.append(np.abs(s * sy.scale_[0]))
        return np.stack(ms, axis=1), np.stack(ss, axis=1)

    # scikit-learn's own outputs agree with the closed forms' values
    m0, s0 = sk_predict(Xq)
    out["csv_pred"] = np.array([rel(mean, m0), rel(std, s0)])
    # fourth-order central differences of scikit-learn's predict through the scalers, step 1e-3 sx.scale_[d]
    fdJ, fdv = np.zeros_like(J), np.zeros_like(dstd)
    for dd in range(D):
        h = FD_H * sx.scale_[dd]
        for w, s in zip(np.array([1.0, -8.0, 8.0, -1.0]) / (12.0 * h), (-2, -1, 1, 2)):
            Q = Xq.copy()
            Q[:, dd] += s * h
            m, sd = sk_predict(Q)
            fdJ[:, :, dd] += w * m
            fdv[:, :, dd] += w * sd ** 2
    out["csv_Xq"], out["csv_mean"], out["csv_std"], out["csv_J"], out["csv_dstd"], out["csv_dvar"] = Xq, mean, std, J, dstd, dvar
    out["csv_sx_mean"], out["csv_sx_scale"] = sx.mean_, sx.scale_
    out["csv_sy_mean"] = np.array([m["sy_mean"] for m in models])
    out["csv_sy_scale"] = np.array([m["sy_scale"] for m in models])
    out["csv_ls"] = np.stack([m["ls"] for m in models])
    out["csv_noise"] = np.array([m["noise"] for m in models])
    out["csv_chk"] = np.stack([colrel(J2, J), colrel(dstd2, dstd), colrel(dvar2, dvar)])
    out["csv_fd"] = np.stack([colrel(fdJ, J), colrel(fdv, 2.0 * std[:, :, None] * dstd)])


def main(path):
    out = {}
    case_ref(out)
    case_csv(out)
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    out = main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "axis_jac_ref.npz"))
    for k, v in out.items():
        print(k, v.shape, v.ravel()[:3])
