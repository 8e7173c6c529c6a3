"""Regenerates tests/golden/paths_ref.npz (NumPy only; reads csv_170501.npz next to it): the inputs, the randomness and the
expected values of the four GPU cases of tests/test_gpu_paths.py, from the dense NumPy form of pathwise conditioning
(DESIGN.md, K10), restated here without BLAS or LAPACK calls, so that the file does not depend on their thread count:

    K = k(X, X) + (noise + alpha) I,   V = K^-1 (Yn (x) 1_S - Phi W - Eps),   Phi = sqrt(2 sf2 / F) cos(X Omega^T + phase)
    f[m, s, p] = y_mean[p] + y_std[p] (k(x_m, X) V[:, s, p] + sqrt(2 sf2 / F) cos(Omega x_m + phase) . W[:, s, p])

Per case c (N, D, F, S, P) the file holds c_X, c_Y, c_Xq (9 rows), c_ls, c_hyper = [sf2, noise, alpha], the randomness c_omega,
c_phase, c_weights (F, S, P), c_eps (N, S, P) from `draw` below (the draw order of paths.draw_path_randomness), c_Xs (S, D),
c_x0 (S, P), c_U (H, D - P), c_lin (P, D), and the expected c_all (9, S, P), c_step (S, P), c_traj (H + 1, S, P).

    python tests/golden/make_golden_paths.py
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "paths_ref.npz")
# (name, N, D, F, S, P, H): nothing a multiple of 64 or 128 / crosses a wave and the 128 padding / CSV rows in the reference's
# shape / S = 1
CASES = (("a", 120, 4, 48, 5, 1, 6), ("b", 130, 4, 64, 70, 3, 5), ("csv", 200, 10, 96, 7, 6, 25), ("one", 128, 3, 16, 1, 2, 4))
ALPHA = 1e-4
MQ = 9


def rbf(A, B, ls, sf2):
    d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
    return sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))


def mm(A, B):
    """A @ B without BLAS (whose blocking, and with it the last bits, follows the thread count): einsum's own loops"""
    return np.einsum("ik,kj->ij", A, B)


def spd_solve(K, R):
    """K^-1 R by a column Cholesky and two substitutions, row by row, for the same reason"""
    n = len(K)
    L = np.zeros_like(K)
    for j in range(n):
        v = K[j:, j] - np.einsum("ik,k->i", L[j:, :j], L[j, :j])
        L[j:, j] = v / np.sqrt(v[0])
    Z = np.zeros_like(R)
    for i in range(n):
        Z[i] = (R[i] - np.einsum("k,kc->c", L[i, :i], Z[:i])) / L[i, i]
    V = np.zeros_like(R)
    for i in range(n - 1, -1, -1):
        V[i] = (Z[i] - np.einsum("k,kc->c", L[i + 1:, i], V[i + 1:])) / L[i, i]
    return V


def draw(rng, N, D, F, S, P, ls, s2):
    omega = rng.standard_normal((F, D)) / ls
    phase = rng.uniform(0.0, 2.0 * np.pi, F)
    weights = rng.standard_normal((F, S, P))
    eps = np.sqrt(s2) * rng.standard_normal((N, S, P))
    return omega, phase, weights, eps


class Form:
    def __init__(self, X, Y, ls, sf2, noise, alpha, omega, phase, weights, eps):
        N, F = len(X), len(omega)
        self.X, self.ls, self.sf2, self.omega, self.phase = X, ls, sf2, omega, phase
        self.ym, self.ys = Y.mean(axis=0), Y.std(axis=0)
        Yn = (Y - self.ym) / self.ys
        self.scale = np.sqrt(2.0 * sf2 / F)
        Phi = self.scale * np.cos(mm(X, omega.T) + phase)
        K = rbf(X, X, ls, sf2) + (noise + alpha) * np.eye(N)
        R = Yn[:, None, :] - np.einsum("nf,fsp->nsp", Phi, weights) - eps
        S, P = weights.shape[1:]
        self.V = spd_solve(K, R.reshape(N, S * P)).reshape(N, S, P)
        self.Ww = self.scale * weights

    def basis(self, Q):
        return rbf(Q, self.X, self.ls, self.sf2), np.cos(mm(Q, self.omega.T) + self.phase)

    def all(self, Q):
        k, c = self.basis(Q)
        return self.ym + self.ys * (np.einsum("mn,nsp->msp", k, self.V) + np.einsum("mf,fsp->msp", c, self.Ww))

    def step(self, Qs):
        k, c = self.basis(Qs)
        return self.ym + self.ys * (np.einsum("sn,nsp->sp", k, self.V) + np.einsum("sf,fsp->sp", c, self.Ww))

    def rollout(self, x0, U, lin):
        traj = [x0]
        for u in U:
            x = traj[-1]
            q = np.concatenate([x, np.broadcast_to(u, (len(x), len(u)))], axis=1)
            traj.append(x + mm(q, lin.T) + self.step(q))
        return np.stack(traj)


def save_npz(path, arrays):
    """np.savez with a fixed time stamp on every member: the same arrays give the same file, byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def build():
    csv = np.load(os.path.join(HERE, "csv_170501.npz"))
    out = {}
    for i, (name, N, D, F, S, P, H) in enumerate(CASES):
        rng = np.random.RandomState(1800 + i)
        if name == "csv":
            X, Y, Xq = csv["X10"][:N], csv["Y6"][:N], csv["Xq10"][:MQ]
            ls, sf2, noise = np.full(D, 0.5), 1.0, 0.1          # train_gp's starting kernel
            dt = 0.02
            lin = np.zeros((P, D))
            lin[0:3, 3:6] = dt * np.eye(3)                       # the double integrator of SimpleQuadrotorGP._nominal_dynamics
            lin[3:6, 6:9] = dt * np.eye(3)
            x0 = np.repeat(X[17:18, :P], S, axis=0)
            U = X[40:40 + H, P:].copy()
        else:
            X = rng.standard_normal((N, D))
            Wm = rng.standard_normal((D, P))
            Y = np.sin(mm(X, Wm)) + 0.5 * X[:, :1] + 0.1 * rng.standard_normal((N, P)) + np.arange(1, P + 1)
            Xq = rng.standard_normal((MQ, D))
            ls, sf2, noise = 1.2 * (1.0 + 0.1 * np.arange(D)), 0.8 + 0.1 * i, 0.05 * (1 + i)
            lin = 0.1 * rng.standard_normal((P, D))
            x0 = 0.5 * rng.standard_normal((S, P))
            U = 0.5 * rng.standard_normal((H, D - P))
        omega, phase, weights, eps = draw(rng, N, D, F, S, P, ls, noise + ALPHA)
        Xs = np.concatenate([Xq, rng.standard_normal((max(S - MQ, 0), D))])[:S]
        form = Form(X, Y, ls, sf2, noise, ALPHA, omega, phase, weights, eps)
        arrays = {"X": X, "Y": Y, "Xq": Xq, "ls": ls, "hyper": np.array([sf2, noise, ALPHA]), "omega": omega, "phase": phase,
                  "weights": weights, "eps": eps, "Xs": Xs, "x0": x0, "U": U, "lin": lin, "all": form.all(Xq),
                  "step": form.step(Xs), "traj": form.rollout(x0, U, lin)}
        for k, v in arrays.items():
            out[f"{name}_{k}"] = np.ascontiguousarray(v, dtype=np.float64)
        print(f"case {name}: N={N} D={D} F={F} S={S} P={P} H={H}  max|all| {np.abs(arrays['all']).max():.3g}  "
              f"max|traj| {np.abs(arrays['traj']).max():.3g}")
    return out


if __name__ == "__main__":
    save_npz(OUT, build())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
