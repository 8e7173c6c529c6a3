"""Regenerates tests/golden/sparse_paths_ref.npz (NumPy only, seeded): the inputs, the randomness and the expected values of
tests/test_gpu_sparse_paths.py and tests/test_sparse_paths_host.py - posterior function draws of the sparse models (DESIGN.md,
K10, "the sparse models") from the dense NumPy form of pathwise conditioning on the inducing variables, in normalised-target
units (yn = (y - y_mean) / y_std with the model's FIXED normalisation, sigma^2 = noise + alpha):

    Luu Luu^T = Kuu + jitter_uu I,  Wuu = Luu^-1,  G = Kuf Kfu,  g = Kuf yn,  B = I + Wuu G Wuu^T / sigma^2 = LB LB^T,
    WS = LB^-1 Wuu,  alpha_u = Wuu^T B^-1 Wuu g / sigma^2
    v_s = alpha_u + WS^T xi_s - Wuu^T (Wuu Phi_Z w_s),   Phi_Z = sqrt(2 sf2 / F) cos(Z Omega^T + phase)
    f_s(x) = k_u(x) v_s + sqrt(2 sf2 / F) cos(Omega x + phase) . w_s,    value = y_mean + y_std f_s(x)

`SparseForm(..., explicit=True)` is that formula with explicit inverses (np.linalg.inv of the two Cholesky factors and of B) and
gives the expected values; `explicit=False` evaluates it a second way, by solves against the factors.  The fixture condition,
asserted per model: the two agree to 1e-10 of each array's largest component and cond(Kuu + jitter_uu I) <= 1e5 - the form is
then determined by its inputs well below the 1e-8 bar of the device tests (the inducing inputs are kept well separated relative
to the length-scales; at cond 8e9 the two ways differ by 3e-6).  A model without rows (n = 0) is the prior: G = 0, g = 0.

Single models, case c (m, D, F, S, P, n): c_Z (m, D), c_X (n, D), c_Y (n, P), c_ls (D,), c_hyper (4,) = [sf2, noise, alpha,
jitter_uu], c_ynorm (2, P) = [y_mean, y_std], c_omega (F, D), c_phase (F,), c_weights (F, S, P), c_xi (m, S, P) (the draw order
of paths.draw_sparse_path_randomness; the last two rounded to float32 and stored so, the expected values computed from the
rounded numbers), c_Xq (9, D), c_Xs (S, D), the expected c_all (9, S, P), c_step (S, P), and c_x0 (S, P), c_U (H, D - P), c_lin
(P, D), c_traj (H + 1, S, P).  Batches, case c (m, D, F, S, B, n): c_Z (B, m, D), c_X (n, D), c_Y (n, B), c_ls (B, D), c_hyper
(B, 4), c_ynorm (2, B), c_omega (B, F, D), c_phase (B, F), c_weights (B, F, S), c_xi (B, m, S), c_out (2, B) = a trainer's
target scaler behind the models, c_Xq, c_Xs, c_all (9, B, S), c_step (S, B) and - unless B > D - c_x0 (S, nx), c_U (H, D - nx),
c_lin (nx, D), c_coord (B,), c_in (2, D) = [in_shift, in_scale], c_traj (H + 1, S, nx), with

    q = [x, U[h]];   z = (q - in_shift) / in_scale;   x <- x + lin q + sum_b e_coord[b] (out_mean_b + out_scale_b value_b(z))

c_growth: the factor by which a 1e-12 relative perturbation of x0 has grown at the end of the horizon in this form.

    python tests/golden/make_golden_sparse_paths.py
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sparse_paths_ref.npz")
# (name, m, D, F, S, P, n, H): nothing a multiple of 64 / C = 210 crosses a 128-column tile, S crosses 64 / m and F each cross one
# 128-tile: the triangular k-ranges of the set-up see two tiles
SINGLES = (("a", 40, 4, 48, 5, 1, 150, 6), ("b", 50, 4, 64, 70, 3, 130, 5), ("g", 150, 4, 130, 3, 2, 300, 4))
# (name, m, D, F, S, B, n, nx, H): own Z per model, input and target scalers / no rows, coordinates without a model / B = 1 /
# the largest B (no rollout: B > D)
BATCHES = (("c", 64, 10, 96, 7, 6, 200, 6, 25), ("d", 33, 10, 32, 9, 4, 0, 6, 5), ("e", 16, 3, 16, 1, 1, 0, 2, 4),
           ("f", 20, 2, 16, 65, 8, 0, 0, 0))
D_COORD = (0, 2, 3, 5)
ALPHA, JITTER_UU = 1e-4, 1e-6
MQ = 9
COND_MAX, AGREE = 1e5, 1e-10


def rbf(A, B, ls, sf2):
    d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


class SparseForm:
    """One sparse model's path set: weights (F, S, P), xi (m, S, P); values in the model's target units.

    .all(Q) (M, S, P); .step(Qs) (S, P); .rollout(x0, U, lin) (H + 1, S, P); .mean(Q) (M, P) and .cov_terms(Q) = (V0^T V0,
    V1^T V1) of the sparse posterior, cov = K** - V0^T V0 + V1^T V1 in normalised units."""

    def __init__(self, Z, X, Y, ls, sf2, noise, alpha, jitter_uu, y_mean, y_std, omega, phase, weights, xi, explicit=True):
        m, F = len(Z), len(omega)
        self.Z, self.ls, self.sf2, self.omega, self.phase = Z, np.asarray(ls, dtype=float), sf2, omega, phase
        self.ym, self.ys = np.atleast_1d(np.asarray(y_mean, dtype=float)), np.atleast_1d(np.asarray(y_std, dtype=float))
        P = len(self.ym)
        s2 = noise + alpha
        Yn = (np.asarray(Y, dtype=float).reshape(len(X), P) - self.ym) / self.ys
        Kuf = rbf(Z, X, self.ls, sf2) if len(X) else np.zeros((m, 0))
        G, g = Kuf @ Kuf.T, Kuf @ Yn
        self.Kuu = rbf(Z, Z, self.ls, sf2) + jitter_uu * np.eye(m)
        Luu = np.linalg.cholesky(self.Kuu)
        self.scale = np.sqrt(2.0 * sf2 / F)
        PhiZ = self.scale * np.cos(Z @ omega.T + phase)
        S = weights.shape[1]
        w2, x2 = weights.reshape(F, S * P), xi.reshape(m, S * P)
        if explicit:
            Wuu = np.linalg.inv(Luu)
            Bm = np.eye(m) + Wuu @ G @ Wuu.T / s2
            LB = np.linalg.cholesky(Bm)
            WS = np.linalg.inv(LB) @ Wuu
            alpha_u = Wuu.T @ (np.linalg.inv(Bm) @ (Wuu @ g / s2))
            V = WS.T @ x2 - Wuu.T @ (Wuu @ (PhiZ @ w2))
            self.Wuu, self.WS = Wuu, WS
        else:
            solve = np.linalg.solve
            A1 = solve(Luu, G)
            Bm = np.eye(m) + solve(Luu, A1.T).T / s2
            LB = np.linalg.cholesky(Bm)
            alpha_u = solve(Luu.T, solve(LB.T, solve(LB, solve(Luu, g) / s2)))
            V = solve(Luu.T, solve(LB.T, x2)) - solve(Luu.T, solve(Luu, PhiZ @ w2))
        self.alpha_u = alpha_u
        self.V = (np.tile(alpha_u, (1, S)) + V).reshape(m, S, P)         # column s P + p: alpha_u's column p
        self.Ww = self.scale * weights

    def cond(self):
        return float(np.linalg.cond(self.Kuu))

    def basis(self, Q):
        return rbf(Q, self.Z, self.ls, self.sf2), np.cos(Q @ self.omega.T + self.phase)

    def all(self, Q):
        k, c = self.basis(Q)
        S, P = self.V.shape[1:]
        f = k @ self.V.reshape(len(self.Z), S * P) + c @ self.Ww.reshape(len(self.omega), S * P)
        return self.ym + self.ys * f.reshape(len(Q), S, P)

    def step(self, Qs):
        k, c = self.basis(Qs)
        return self.ym + self.ys * (np.einsum("sn,nsp->sp", k, self.V) + np.einsum("sf,fsp->sp", c, self.Ww))

    def rollout(self, x0, U, lin):
        S, P = self.V.shape[1:]
        traj = [np.broadcast_to(x0, (S, P))]
        for u in U:
            x = traj[-1]
            q = np.concatenate([x, np.broadcast_to(u, (S, len(u)))], axis=1)
            traj.append(x + q @ lin.T + self.step(q))
        return np.stack(traj)

    def mean(self, Q):
        return self.ym + self.ys * (rbf(Q, self.Z, self.ls, self.sf2) @ self.alpha_u)

    def cov_terms(self, Q):
        ku = rbf(Q, self.Z, self.ls, self.sf2)
        V0, V1 = self.Wuu @ ku.T, self.WS @ ku.T
        return V0.T @ V0, V1.T @ V1

    def ensemble_cov(self, Q):
        """(A A^T, B B^T): the closed-form covariance of f(Q) over xi ~ N(0, I_m), w ~ N(0, I_F) is their sum"""
        ku, c = self.basis(Q)
        PhiZ = self.scale * np.cos(self.Z @ self.omega.T + self.phase)
        A = self.scale * c - ku @ self.Wuu.T @ self.Wuu @ PhiZ
        Bq = ku @ self.WS.T
        return A @ A.T, Bq @ Bq.T


class SparseBatchForm:
    """B single-output sparse models, each with its own Z: Z (B, m, D), ls (B, D), hyper (B, 4), ynorm (2, B), weights (B, F, S),
    xi (B, m, S), out = (out_mean (B,), out_scale (B,)) or None.  .all(Q) (M, B, S); .step(Qs) (S, B);
    .rollout(x0, U, lin, coord, in_scaler) (H + 1, S, nx)."""

    def __init__(self, Z, X, Y, ls, hyper, ynorm, omega, phase, weights, xi, out=None, explicit=True):
        B = len(ls)
        self.forms = [SparseForm(Z[b], X, Y[:, b:b + 1], ls[b], hyper[b, 0], hyper[b, 1], hyper[b, 2], hyper[b, 3], ynorm[0, b],
                                 ynorm[1, b], omega[b], phase[b], weights[b][:, :, None], xi[b][:, :, None], explicit)
                      for b in range(B)]
        self.out_mean, self.out_scale = (np.zeros(B), np.ones(B)) if out is None else (np.asarray(out[0]), np.asarray(out[1]))

    def all(self, Q):
        return np.stack([self.out_mean[b] + self.out_scale[b] * f.all(Q)[:, :, 0] for b, f in enumerate(self.forms)], axis=1)

    def step(self, Qs):
        return np.stack([self.out_mean[b] + self.out_scale[b] * f.step(Qs)[:, 0] for b, f in enumerate(self.forms)], axis=1)

    def rollout(self, x0, U, lin, coord=None, in_scaler=None):
        B, nx, D = len(self.forms), lin.shape[0], lin.shape[1]
        coord = np.arange(B) if coord is None else np.asarray(coord, dtype=int)
        shift, scale = (np.zeros(D), np.ones(D)) if in_scaler is None else in_scaler
        S = self.forms[0].V.shape[1]
        traj = [np.broadcast_to(x0, (S, nx))]
        for u in U:
            x = traj[-1]
            q = np.concatenate([x, np.broadcast_to(u, (S, len(u)))], axis=1)
            nxt = x + q @ lin.T
            nxt[:, coord] += self.step((q - shift) / scale)
            traj.append(nxt)
        return np.stack(traj)


def draw(rng, m, D, F, S, P, ls):
    """the order of paths.draw_sparse_path_randomness"""
    omega = rng.standard_normal((F, D)) / ls
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    weights = rng.standard_normal((F, S, P))
    xi = rng.standard_normal((m, S, P))
    return omega, phase, weights, xi


def f32(a):
    return a.astype(np.float32).astype(np.float64)


def growth(roll, x0):
    """the factor by which a 1e-12 relative perturbation of x0 has grown at the end of the horizon"""
    base = roll(x0)
    pert = roll(x0 * (1.0 + 1e-12) + 1e-12)
    d0 = np.max(np.abs(pert[0] - base[0]))
    return float(np.max(np.abs(pert[-1] - base[-1])) / d0)


def save_npz(path, arrays):
    """np.savez with a fixed time stamp on every member"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def well_determined(tag, first, second, keys):
    """the fixture condition: both ways agree to AGREE, every Kuu + jitter_uu I has a condition number of at most COND_MAX"""
    worst = max(relerr(second[k], first[k]) for k in keys)
    assert worst <= AGREE, (tag, worst)
    return worst


def build():
    out = {}
    for i, (name, m, D, F, S, P, n, H) in enumerate(SINGLES):
        rng = np.random.RandomState(2000 + i)
        ls = 1.0 * (1.0 + 0.1 * np.arange(D))
        sf2, noise = 0.9, 0.05
        # inducing inputs well separated relative to the length-scales: a spread of 2 in every coordinate
        Z = 2.0 * rng.standard_normal((m, D))
        X = 2.0 * rng.standard_normal((n, D))
        Wm = rng.standard_normal((D, P))
        Y = np.sin(0.5 * X @ Wm) + 0.25 * X[:, :1] + 0.1 * rng.standard_normal((n, P)) + np.arange(1, P + 1)
        ynorm = np.stack([Y.mean(axis=0) + 0.05, 1.1 * Y.std(axis=0)])      # a fixed normalisation, close to the rows' own
        Xq = 2.0 * rng.standard_normal((MQ, D))
        omega, phase, weights, xi = draw(rng, m, D, F, S, P, ls)
        weights, xi = f32(weights), f32(xi)
        Xs = np.concatenate([Xq, 2.0 * rng.standard_normal((max(S - MQ, 0), D))])[:S]
        lin = 0.1 * rng.standard_normal((P, D))
        x0 = 0.5 * rng.standard_normal((S, P))
        U = 0.5 * rng.standard_normal((H, D - P))
        args = (Z, X, Y, ls, sf2, noise, ALPHA, JITTER_UU, ynorm[0], ynorm[1], omega, phase, weights, xi)
        form, other = SparseForm(*args), SparseForm(*args, explicit=False)
        # (the state lives near 0, the targets near 1 .. P: the rollout takes the model's values as they are)
        vals = [{"all": f.all(Xq), "step": f.step(Xs), "traj": f.rollout(x0, U, lin)} for f in (form, other)]
        agree = well_determined(name, vals[0], vals[1], ("all", "step", "traj"))
        cond = form.cond()
        assert cond <= COND_MAX, (name, cond)
        gr = growth(lambda x: form.rollout(x, U, lin), x0)
        arrays = {"Z": Z, "X": X, "Y": Y, "ls": ls, "hyper": np.array([sf2, noise, ALPHA, JITTER_UU]), "ynorm": ynorm, "omega": omega,
                  "phase": phase, "weights": weights, "xi": xi, "Xq": Xq, "Xs": Xs, "x0": x0, "U": U, "lin": lin,
                  "growth": np.array(gr), **vals[0]}
        for k, v in arrays.items():
            out[f"{name}_{k}"] = np.ascontiguousarray(v, dtype=np.float32 if k in ("weights", "xi") else np.float64)
        print(f"case {name}: m={m} D={D} F={F} S={S} P={P} n={n} H={H}  cond {cond:.3g}  two ways differ by {agree:.1e}  "
              f"growth of 1e-12 over the horizon {gr:.2f}x  max|all| {np.abs(vals[0]['all']).max():.3g}")
    for i, (name, m, D, F, S, B, n, nx, H) in enumerate(BATCHES):
        rng = np.random.RandomState(2100 + i)
        # distinct per model: length-scales, signal variance, noise, inducing inputs
        base = 2.0 if D == 10 else 1.0
        ls = np.stack([base * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b) for b in range(B)])
        hyper = np.stack([[0.8 + 0.1 * b, 0.05 * (1 + b), ALPHA, JITTER_UU] for b in range(B)])
        spread = 1.0 if D == 10 else 3.0
        Z = spread * rng.standard_normal((B, m, D))
        X = spread * rng.standard_normal((n, D))
        Wm = rng.standard_normal((D, B))
        Y = np.sin(0.3 * X @ Wm) + 0.2 * X[:, :1] + 0.1 * rng.standard_normal((n, B)) + 0.3 * np.arange(1, B + 1)
        ynorm = np.stack([0.3 * np.arange(1, B + 1) + 0.02, np.full(B, 0.8) + 0.05 * np.arange(B)])
        Xq = spread * rng.standard_normal((MQ, D))
        in_shift, in_scale = 0.2 * rng.standard_normal(D), 0.5 + rng.uniform(0.0, 1.0, D)
        outs = np.stack([0.01 * rng.standard_normal(B) - 0.02 * np.arange(1, B + 1), 0.05 + 0.01 * np.arange(B)])
        coord = np.array(D_COORD) if name == "d" else np.arange(B)
        om, ph, w, x = zip(*[draw(rng, m, D, F, S, 1, ls[b]) for b in range(B)])
        omega, phase = np.stack(om), np.stack(ph)
        weights, xi = f32(np.stack(w)[:, :, :, 0]), f32(np.stack(x)[:, :, :, 0])
        Xs = np.concatenate([Xq, spread * rng.standard_normal((max(S - MQ, 0), D))])[:S]
        args = (Z, X, Y, ls, hyper, ynorm, omega, phase, weights, xi, outs)
        form, other = SparseBatchForm(*args), SparseBatchForm(*args, explicit=False)
        roll = None
        if H:
            if name == "c":
                dt = 0.02
                lin = np.zeros((nx, D))
                lin[0:3, 3:6] = dt * np.eye(3)                       # the double integrator of GPTrainer._nominal_dynamics
                lin[3:6, 6:9] = dt * np.eye(3)
            else:
                lin = 0.1 * rng.standard_normal((nx, D))
            # raw units: the scaled state starts where the inducing inputs are
            x0 = in_shift[:nx] + in_scale[:nx] * 0.5 * rng.standard_normal((S, nx))
            U = in_shift[nx:] + in_scale[nx:] * 0.5 * rng.standard_normal((H, D - nx))
            roll = lambda f, x: f.rollout(x, U, lin, coord, (in_shift, in_scale))      # noqa: E731
        vals = [{"all": f.all(Xq), "step": f.step(Xs), **({"traj": roll(f, x0)} if H else {})} for f in (form, other)]
        agree = well_determined(name, vals[0], vals[1], tuple(vals[0]))
        cond = max(f.cond() for f in form.forms)
        assert cond <= COND_MAX, (name, cond)
        arrays = {"Z": Z, "X": X, "Y": Y, "ls": ls, "hyper": hyper, "ynorm": ynorm, "omega": omega, "phase": phase,
                  "weights": weights, "xi": xi, "out": outs, "Xq": Xq, "Xs": Xs, **vals[0]}
        gr = float("nan")
        if H:
            gr = growth(lambda x: roll(form, x), x0)
            arrays.update({"x0": x0, "U": U, "lin": lin, "coord": coord.astype(np.float64), "in": np.stack([in_shift, in_scale]),
                           "growth": np.array(gr)})
        for k, v in arrays.items():
            out[f"{name}_{k}"] = np.ascontiguousarray(v, dtype=np.float32 if k in ("weights", "xi") else np.float64)
        print(f"case {name}: m={m} D={D} F={F} S={S} B={B} n={n} nx={nx} H={H}  largest cond {cond:.3g}  two ways differ by "
              f"{agree:.1e}  growth {gr:.2f}x  max|all| {np.abs(vals[0]['all']).max():.3g}")
    return out


if __name__ == "__main__":
    save_npz(OUT, build())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
