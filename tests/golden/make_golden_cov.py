"""Regenerate tests/golden/cov_ref.npz: scikit-learn's joint posterior (predict(X, return_cov=True)) and sample_y at fixed
hyper-parameters (optimizer=None) on the committed flight data (csv_170501.npz).  Needs scikit-learn only.

    python tests/golden/make_golden_cov.py [out.npz]

Cases (prefix_*): ka1 - RBF(0.5) + White(0.1), alpha 1e-4, normalize_y, D = 10, P = 6 on the 64 Xq10 queries; one - the
same kernel, one 1-D target, normalize_y=False; ard - C(2.0) * RBF(ARD) + White(0.05), 2-D target with one column;
prior - the unfitted ka1 kernel on 25 queries; sample_y of `one` and `ka1` on the first 25 queries (8 samples,
random_state 0) with the smallest relative gap between consecutive singular values of each covariance drawn from
(multivariate_normal draws through an SVD: where that gap is tiny the singular vectors, and with them the samples, are
not determined by the covariance to the precision of its entries)."""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"        # one BLAS thread: the same bits on every run

import numpy as np  # noqa: E402
from sklearn.gaussian_process import GaussianProcessRegressor  # noqa: E402
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NQ_SAMPLE = 25
N_SAMPLES = 8


def min_rel_gap(cov):
    s = np.linalg.svd(cov, compute_uv=False)
    return float(np.min(-np.diff(s)) / s[0])


def main(path):
    d = np.load(os.path.join(HERE, "csv_170501.npz"))
    X, Y, Xq = d["X10"], d["Y6"], d["Xq10"]
    out = {}
    k1 = RBF(0.5) + WhiteKernel(0.1)
    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=True, optimizer=None).fit(X, Y)
    out["ka1_mean"], out["ka1_cov"] = g.predict(Xq, return_cov=True)
    out["ka1_samples"] = g.sample_y(Xq[:NQ_SAMPLE], N_SAMPLES, random_state=0)
    _, c = g.predict(Xq[:NQ_SAMPLE], return_cov=True)
    out["ka1_gap"] = np.array([min_rel_gap(c[..., p]) for p in range(c.shape[2])])

    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=False, optimizer=None).fit(X, Y[:, 0])
    out["one_mean"], out["one_cov"] = g.predict(Xq, return_cov=True)
    out["one_samples"] = g.sample_y(Xq[:NQ_SAMPLE], N_SAMPLES, random_state=0)
    _, c = g.predict(Xq[:NQ_SAMPLE], return_cov=True)
    out["one_gap"] = np.array([min_rel_gap(c)])

    ls = np.linspace(0.4, 1.3, X.shape[1])
    k3 = ConstantKernel(2.0) * RBF(ls) + WhiteKernel(0.05)
    g = GaussianProcessRegressor(kernel=k3, alpha=1e-5, normalize_y=True, optimizer=None).fit(X, Y[:, [2]])
    out["ard_ls"] = ls
    out["ard_mean"], out["ard_cov"] = g.predict(Xq, return_cov=True)

    g = GaussianProcessRegressor(kernel=k1, alpha=1e-4, normalize_y=True, optimizer=None)
    out["prior_mean"], out["prior_cov"] = g.predict(Xq[:NQ_SAMPLE], return_cov=True)
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    out = main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "cov_ref.npz"))
    for k, v in out.items():
        print(k, v.shape, v.ravel()[:3])
