"""Writes tests/golden/sparse_z_ref.npz: the gradient of the sparse GP's collapsed bound with respect to the inducing inputs Z, the
column pass behind it, and a small case of training Z ("training Z").

NumPy and SciPy only, seeded, reproduces its file bit for bit.  The inputs are those of tests/golden/sparse_train_ref.npz (read
from there, not copied); the functions of make_golden_sparse_train.py are imported.  Every dL/dZ is computed twice,

* by the assembly form the library uses (include/gpk.h, gpk_sparse_eval_z): T = Q o Kfu with Q = [Kfu | Yn] C, GammaK = dL/dKuu,
      dL/dz_id = (U_id + V_id) / ls_d,  U_id = sum_n T_ni (x_nd / ls_d - z_id / ls_d),
      V_id = 2 sum_j GammaK_ij Kuu0_ij (z_jd / ls_d - z_id / ls_d);
* by the dense N x N form: dL/dKfu = 2 M A^T, dL/dKuu = -A M A^T of `grad_dense`, chained through the same two derivatives of
  the RBF,

and against central differences of `bound_value` on a seeded sample of 16 entries.  The file is written only if the two forms
agree to 1e-6 of the largest component and the differences to 1e-5; the measured agreements are stored.  (Case A's Kuu has
jitter_uu = 1.3e-8: its conditioning, not the formula, sets the two forms' 2e-8.)

The step of the differences is 1e-5 on case A.  The training case at its start point - length-scales three times the true ones
on 64 inducing inputs - is so ill-conditioned that `bound_value` itself carries rounding noise of about 1e-8 there (moving Z by
1e-13 moves it by 7e-9; its value is -1267): at h = 1e-5 that noise alone is 1e-8 / 2e-5 = 5e-4, 1.4e-4 of the largest
component 3.7, and the differences say nothing.  The step that balances noise against the h^2 truncation, the cube root of
3 noise / |third derivative| with a third derivative of order 10, is about 1e-3; that step is used there (measured over 1e-5 ..
3e-3: 1.4e-4, 4.9e-5, 1.4e-5, 5.8e-6, 2.9e-6 at 1e-3, 1.6e-5).  The gate is the same 1e-5.

    python tests/golden/make_golden_sparse_z.py
"""
import os
import sys

import numpy as np
from scipy.linalg import cho_solve, cholesky
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sparse_train as W  # noqa: E402

FORMS_GATE, FD_GATE, FD_STEP, FD_STEP_ILL, FD_SAMPLE = 1e-6, 1e-5, 1e-5, 1e-3, 16


def scaled_diff(A, B, ls):
    """a_nd / ls_d - b_id / ls_d as (n, i, d), by differences of the divided coordinates"""
    return (A / ls)[:, None, :] - (B / ls)[None, :, :]


def zpass_sums(X, Yn, Z, ls, sf2, Cm):
    """The column pass: R[i][d] = sum_n T_ni (x_nd / ls_d - z_id / ls_d) for d < D and R[i][D] = sum_n T_ni, T = Q o Kfu,
    Q = [Kfu | Yn] Cm; and the sums of the absolute values of the same terms.  Both (m, D + 1)."""
    Kfu = W.rbf(X, Z, ls, sf2)
    T = (np.hstack([Kfu, Yn]) @ Cm) * Kfu
    terms = T[:, :, None] * scaled_diff(X, Z, ls)
    R = np.concatenate([terms.sum(axis=0), T.sum(axis=0)[:, None]], axis=1)
    Ra = np.concatenate([np.abs(terms).sum(axis=0), np.abs(T).sum(axis=0)[:, None]], axis=1)
    return R, Ra


def kuu_term(Z, ls, sf2, GK):
    """V_id = 2 sum_j GK_ij Kuu0_ij (z_jd / ls_d - z_id / ls_d)"""
    Kuu0 = W.rbf(Z, Z, ls, sf2)
    return 2.0 * np.einsum("ij,jid->id", GK * Kuu0, scaled_diff(Z, Z, ls))


def gradz_assembly(X, Yn, Z, ls, sf2, noise, jitter, jit):
    pt = W.partials(X, Yn, Z, ls, sf2, noise, jitter, jit)
    R, _ = zpass_sums(X, Yn, Z, ls, sf2, W.coef_matrix(pt))
    return (R[:, :-1] + kuu_term(Z, ls, sf2, pt["GK"])) / ls


def gradz_dense(X, Yn, Z, ls, sf2, noise, jitter, jit):
    N, m, P = len(X), len(Z), Yn.shape[1]
    s2 = noise + jitter
    Kfu = W.rbf(X, Z, ls, sf2)
    Kuu0 = W.rbf(Z, Z, ls, sf2)
    A = cho_solve((cholesky(Kuu0 + jit * np.eye(m), lower=True), True), Kfu.T)
    Ci = cho_solve((cholesky(Kfu @ A + s2 * np.eye(N), lower=True), True), np.eye(N))
    a = Ci @ Yn
    M = 0.5 * (a @ a.T - P * Ci) + P / (2 * s2) * np.eye(N)
    dKfu = 2.0 * M @ A.T
    dKuu = -A @ M @ A.T
    U = np.einsum("ni,nid->id", dKfu * Kfu, scaled_diff(X, Z, ls))
    return (U + kuu_term(Z, ls, sf2, dKuu)) / ls


def gradz_central(X, Yn, Z, ls, sf2, noise, jitter, jit, entries, h=FD_STEP):
    out = np.empty(len(entries))
    for k, (i, d) in enumerate(entries):
        v = []
        for s in (1.0, -1.0):
            Zs = Z.copy()
            Zs[i, d] += s * h
            v.append(W.bound_value(X, Yn, Zs, ls, sf2, noise, jitter, jit))
        out[k] = (v[0] - v[1]) / (2 * h)
    return out


def fd_entries(seed, m, D, count=FD_SAMPLE):
    flat = np.sort(np.random.default_rng(seed).permutation(m * D)[:min(count, m * D)])
    return [(int(e // D), int(e % D)) for e in flat]


def checked_gradz(name, X, Yn, Z, ls, sf2, noise, jitter, jit, seed, h=FD_STEP):
    ga = gradz_assembly(X, Yn, Z, ls, sf2, noise, jitter, jit)
    gd = gradz_dense(X, Yn, Z, ls, sf2, noise, jitter, jit)
    ent = fd_entries(seed, *Z.shape)
    gc = gradz_central(X, Yn, Z, ls, sf2, noise, jitter, jit, ent, h)
    top = np.max(np.abs(ga))
    e_forms = float(np.max(np.abs(ga - gd)) / top)
    e_fd = float(np.max(np.abs(gc - np.array([ga[i, d] for i, d in ent]))) / top)
    print("%s: dL/dZ, assembly against dense form %.1e, central differences (h = %g) on %d entries %.1e (largest component %.3e)" % (
        name, e_forms, h, len(ent), e_fd, top))
    assert e_forms < FORMS_GATE, (name, "the two forms", e_forms)
    assert e_fd < FD_GATE, (name, "central differences", e_fd)
    return ga, e_forms, e_fd


def train_small(X, Yn, Z0, t0, jitter, jit, with_z):
    """L-BFGS-B on the NumPy bound from theta = t0 ([sf2, ls_0, ls_1, noise], logs): over theta alone, or over [theta, Z]."""
    lo, hi = np.log(1e-5), np.log(1e5)
    m, D = Z0.shape

    def obj(v):
        e = np.exp(v[:4])
        Z = v[4:].reshape(m, D) if with_z else Z0
        try:
            b = W.bound_value(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
            g, _, _ = W.grad_assembly(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit)
            gt = np.array([g[3], g[0], g[1], g[2]])
            if with_z:
                gt = np.concatenate([gt, gradz_assembly(X, Yn, Z, e[1:3], e[0], e[3], jitter, jit).ravel()])
        except np.linalg.LinAlgError:
            return np.inf, np.zeros_like(v)
        return -b, -gt

    v0 = np.concatenate([t0, Z0.ravel()]) if with_z else t0.copy()
    bounds = [(lo, hi)] * 4 + ([(None, None)] * Z0.size if with_z else [])
    res = minimize(obj, v0, method="L-BFGS-B", jac=True, bounds=bounds)
    return res


def main():
    src = np.load(os.path.join(HERE, "sparse_train_ref.npz"))
    out = {}
    # ---- case A (ARD) and its isotropic variant ------------------------------------------------------------------------
    X, Y, Z, ls = src["A_X"], src["A_Y"], src["A_Z"], src["A_ls"]
    sf2, noise, alpha, jit = src["A_hyper"]
    Yn = (Y - src["A_y_mean"]) / src["A_y_std"]
    g, ef, ed = checked_gradz("case A", X, Yn, Z, ls, sf2, noise, alpha, jit, 850)
    out.update(A_gradZ=g, A_gradZ_agree=np.array([ef, ed]))
    iso = np.full(X.shape[1], float(src["Aiso_ls"][0]))
    g, ef, ed = checked_gradz("case A, isotropic", X, Yn, Z, iso, sf2, noise, alpha, jit, 851)
    out.update(Aiso_gradZ=g, Aiso_gradZ_agree=np.array([ef, ed]))
    # the column pass alone, on the random coefficient matrix of the existing fixture
    R, Ra = zpass_sums(X, Yn, Z, ls, sf2, src["A_C"])
    out.update(A_zpass=R, A_zpass_abs=Ra)
    # ---- the 600-row training case at its start point (m = 64, jitter_uu = 1e-4) ------------------------------------------
    X, Y, Z = src["T_X"], src["T_Y"], src["T_Z"]
    Yn = (Y - src["T_y_mean"]) / src["T_y_std"]
    sf20, l0, l1, noise0 = src["T_start"]
    jitter, jit = src["T_hyper"]
    g, ef, ed = checked_gradz("training case, start", X, Yn, Z, np.array([l0, l1]), sf20, noise0, jitter, jit, 852, h=FD_STEP_ILL)
    out.update(T_gradZ=g, T_gradZ_agree=np.array([ef, ed]))
    # ---- training Z: the same rows, m = 16 inducing inputs ------------------------------------------------------------------
    Z16 = X[np.sort(np.random.default_rng(5).permutation(len(X))[:16])].copy()
    t0 = np.log(src["T_start"])
    b0 = W.bound_value(X, Yn, Z16, np.array([l0, l1]), sf20, noise0, jitter, jit)
    rt = train_small(X, Yn, Z16, t0, jitter, jit, False)
    rz = train_small(X, Yn, Z16, t0, jitter, jit, True)
    print("training Z, m = 16: bound %.6f at the start; L-BFGS-B over the kernel %.6f (%d evaluations), over the kernel and Z %.6f "
          "(%d evaluations)" % (b0, -rt.fun, rt.nfev, -rz.fun, rz.nfev))
    assert -rz.fun > -rt.fun > b0
    out.update(Z16_Z=Z16, Z16_bound_start=np.array(b0), Z16_bound_theta_opt=np.array(-rt.fun), Z16_theta_opt=rt.x,
               Z16_bound_z_opt=np.array(-rz.fun), Z16_z_opt_theta=rz.x[:4], Z16_z_opt_Z=rz.x[4:].reshape(Z16.shape))
    path = os.path.join(HERE, "sparse_z_ref.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
