#!/usr/bin/env python3
"""Gradient fixtures (run ONCE in the build container; the files of the earlier make_golden*.py stay as they are).

Imports scikit-learn 1.7.2 and the reference's ROS-package GP module from /root/reference (read-only; `rclpy` and
`std_msgs` are stood in for exactly as tests/golden/make_golden_r5.py does) and freezes numbers only.  The data are row
indices into tests/golden/csv_170501.npz (X10[:, :9] as inputs, target columns of Y6) or the deterministic
`oracle.gp_oracle.synthetic_problem`, so the fixture holds no copy of them:

  grad_ref.npz
    sk_*   scikit-learn's `GaussianProcessRegressor.log_marginal_likelihood(theta, eval_gradient=True)` with the constant
           FREE: `C(1.3) * RBF(ls) + WhiteKernel(0.05)`, `alpha = 1e-4`, `normalize_y=True`, `optimizer=None`, on the
           500 rows `sk_rows`; isotropic (ls 1.5) and ARD (ls 1.5 (1 + 0.1 d)); P = 1 (Y6[:, 3], 1-D y) and P = 3
           (Y6[:, 3:6]); at theta0 = kernel.theta and at theta0 + `sk_dtheta` (iso: the first three entries).  theta order
           is scikit-learn's: [log sf2, log ls..., log noise].
    pk_*   the reference `GaussianProcess.log_marginal_likelihood()` (gaussian_process.py:243-265) after `fit()` at
           theta0 = log [ls, sf2, noise] = log [1.5, 0.8, 0.05] and at theta0 + k h e_i, k in (-2, -1, 1, 2), h = 1e-3,
           for the three log-parameters: the reference's own objective, from which a test forms a 4th-order central
           difference.  output_dim 1 and 3: the first N CSV rows (Y6[:, 3] / Y6[:, 3:6]); output_dim 12:
           `synthetic_problem(N, 1, D=9, P=12)`.  N in (120, 257, 1000).  Arrays pk_lml0_P{P}_N{N} () and
           pk_lml_P{P}_N{N} (3, 4) [parameter, k].

    python tests/golden/make_golden_grad.py

The archive is written with fixed member timestamps, so a rerun reproduces the file bit for bit.
Nothing here is reference source: the fixture holds indices, parameters and the values the reference computed.
"""
import io
import os
import sys
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SK_ROWS = np.arange(0, 1000, 2)
SK_DTHETA = np.array([0.25, -0.3, 0.2, 0.15, -0.1, 0.3, -0.25, 0.1, 0.05, -0.2, 0.4])
PK_THETA0 = np.log([1.5, 0.8, 0.05])
PK_H = 1e-3
PK_KS = (-2, -1, 1, 2)
PK_NS = (120, 257, 1000)
PK_PS = (1, 3, 12)


def pk_data(csv, N, P):
    if P == 12:
        from oracle.gp_oracle import synthetic_problem
        X, Y, _ = synthetic_problem(N, 1, D=9, P=12)
        return X, Y
    X = csv["X10"][:N, :9]
    Y = csv["Y6"][:N, 3:3 + P]
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def sk_case(csv, ard, P):
    X = csv["X10"][SK_ROWS, :9]
    y = csv["Y6"][SK_ROWS, 3] if P == 1 else csv["Y6"][SK_ROWS, 3:6]
    ls = 1.5 * (1.0 + 0.1 * np.arange(9)) if ard else 1.5
    return X, y, ls


def sklearn_part(csv):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel

    out = {"sk_rows": SK_ROWS, "sk_dtheta": SK_DTHETA, "sk_sf2": np.array(1.3), "sk_noise": np.array(0.05),
           "sk_alpha": np.array(1e-4)}
    for ard in (0, 1):
        for P in (1, 3):
            X, y, ls = sk_case(csv, ard, P)
            kern = ConstantKernel(1.3) * RBF(ls) + WhiteKernel(0.05)
            g = GaussianProcessRegressor(kernel=kern, alpha=1e-4, normalize_y=True, optimizer=None).fit(X, y)
            th0 = g.kernel_.theta.copy()
            thetas = np.stack([th0, th0 + SK_DTHETA[: th0.size]])
            lml, grad = [], []
            for th in thetas:
                l, gr = g.log_marginal_likelihood(th, eval_gradient=True)
                lml.append(l)
                grad.append(gr)
            tag = f"ard{ard}_P{P}"
            out[f"sk_theta_{tag}"] = thetas
            out[f"sk_lml_{tag}"] = np.array(lml)
            out[f"sk_grad_{tag}"] = np.array(grad)
    return out


def package_part(csv):
    from make_golden_r5 import import_reference_package_gp

    pkg_gp, _ = import_reference_package_gp()

    def lml_at(X, Y, theta):
        gp = pkg_gp.GaussianProcess(input_dim=9, output_dim=Y.shape[1])
        gp.X_train, gp.Y_train = X.copy(), Y.copy()
        gp.kernel.length_scale, gp.kernel.signal_variance, gp.noise_variance = (float(v) for v in np.exp(theta))
        gp.fit()
        return float(gp.log_marginal_likelihood())

    out = {"pk_theta0": PK_THETA0, "pk_h": np.array(PK_H), "pk_ks": np.array(PK_KS), "pk_N": np.array(PK_NS),
           "pk_P": np.array(PK_PS)}
    for P in PK_PS:
        for N in PK_NS:
            X, Y = pk_data(csv, N, P)
            out[f"pk_lml0_P{P}_N{N}"] = np.array(lml_at(X, Y, PK_THETA0))
            tab = np.empty((3, len(PK_KS)))
            for i in range(3):
                for j, k in enumerate(PK_KS):
                    th = PK_THETA0.copy()
                    th[i] += k * PK_H
                    tab[i, j] = lml_at(X, Y, th)
            out[f"pk_lml_P{P}_N{N}"] = tab
    return out


def save_npz_stable(path, arrays):
    """np.savez_compressed with fixed member timestamps (np.savez stamps every member with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    csv = {k: d[k] for k in d.files}
    out = sklearn_part(csv)
    out.update(package_part(csv))
    path = os.path.join(HERE, "grad_ref.npz")
    save_npz_stable(path, out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
