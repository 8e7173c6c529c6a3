"""Regenerates tests/golden/axis_paths_ref.npz (NumPy only; reads csv_170501.npz next to it): the inputs, the randomness and the
expected values of the GPU cases of tests/test_gpu_axis_paths.py - posterior function draws of the per-axis batch (DESIGN.md,
K10, "the per-axis batch"): B single-output models on shared inputs, each with its own length-scales, signal variance and noise
- from the dense NumPy form of pathwise conditioning, restated here without BLAS or LAPACK calls, so that the file does not
depend on their thread count.  Per model b (targets normalised column by column, normalize_y=True):

    K_b = k_b(X, X) + (noise_b + alpha) I,   V_b = K_b^-1 (yn_b 1_S^T - Phi_b W_b - Eps_b),
    Phi_b = sqrt(2 sf2_b / F) cos(X Omega_b^T + phase_b)
    f[m, b, s] = y_mean_b + y_std_b (k_b(x_m, X) V_b[:, s] + sqrt(2 sf2_b / F) cos(Omega_b x_m + phase_b) . W_b[:, s])

and the value served is out_mean_b + out_scale_b f (a trainer's target scaler; identity except in case csv).  A rollout, in raw
units, state of nx coordinates, model b feeding coordinate coord[b]:

    q = [x, U[h]];   z = (q - in_shift) / in_scale;   x <- x + lin q + sum_b e_coord[b] value_b(z)

Per case c (N, D, F, S, B) the file holds c_X (N, D: what the models are fitted on), c_Y (N, B), c_Xq (9, D), c_ls (B, D),
c_hyper (B, 3) = [sf2, noise, alpha] per model, the randomness c_omega (B, F, D), c_phase (B, F), c_weights (B, F, S), c_eps
(B, N, S) from `draw` below (the draw order of paths.draw_batch_path_randomness; the last two - the bulk of the file - rounded to
float32 and stored as float32, the expected values computed from the rounded numbers), c_Xs (S, D), c_out (2, B) = [out_mean,
out_scale], the expected c_all (9, B, S) and c_step (S, B), and - every case but `eight`, whose B exceeds its D - c_x0 (S, nx),
c_U (H, D - nx), c_lin (nx, D), c_coord (B,), c_in (2, D) = [in_shift, in_scale] and the expected c_traj (H + 1, S, nx).

    python tests/golden/make_golden_axis_paths.py
"""
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "axis_paths_ref.npz")
# (name, N, D, F, S, B, nx, H): nothing a multiple of 64 / two path blocks, S not a multiple of 8 / CSV rows, input and target
# scalers / coordinates without a model / B = 1 / the largest B (no rollout: B > D)
CASES = (("a", 120, 4, 48, 5, 2, 3, 6), ("b", 130, 4, 64, 70, 3, 3, 5), ("csv", 200, 10, 96, 7, 6, 6, 25),
         ("gap", 96, 10, 32, 9, 4, 6, 5), ("one", 128, 3, 16, 1, 1, 2, 4), ("eight", 64, 2, 16, 65, 8, 0, 0))
GAP_COORD = (0, 2, 3, 5)
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


def draw(rng, N, D, F, S, ls, s2):
    """model by model from the one generator, each in the order of paths.draw_path_randomness with P = 1"""
    om, ph, w, e = [], [], [], []
    for b in range(len(ls)):
        om.append(rng.standard_normal((F, D)) / ls[b])
        ph.append(rng.uniform(0.0, 2.0 * np.pi, F))
        w.append(rng.standard_normal((F, S, 1))[:, :, 0])
        e.append((np.sqrt(s2[b]) * rng.standard_normal((N, S, 1)))[:, :, 0])
    return np.stack(om), np.stack(ph), np.stack(w), np.stack(e)


class Model:
    """one model's path set: weights (F, S), eps (N, S); values (M, S) in the model's target units"""

    def __init__(self, X, y, ls, sf2, noise, alpha, omega, phase, weights, eps):
        N, F = len(X), len(omega)
        self.X, self.ls, self.sf2, self.omega, self.phase = X, ls, sf2, omega, phase
        self.ym, self.ys = y.mean(), y.std()
        yn = (y - self.ym) / self.ys
        self.scale = np.sqrt(2.0 * sf2 / F)
        Phi = self.scale * np.cos(mm(X, omega.T) + phase)
        K = rbf(X, X, ls, sf2) + (noise + alpha) * np.eye(N)
        self.V = spd_solve(K, yn[:, None] - mm(Phi, weights) - eps)
        self.Ww = self.scale * weights

    def basis(self, Q):
        return rbf(Q, self.X, self.ls, self.sf2), np.cos(mm(Q, self.omega.T) + self.phase)

    def all(self, Q):
        k, c = self.basis(Q)
        return self.ym + self.ys * (mm(k, self.V) + mm(c, self.Ww))

    def step(self, Qs):
        k, c = self.basis(Qs)
        return self.ym + self.ys * (np.einsum("sn,ns->s", k, self.V) + np.einsum("sf,fs->s", c, self.Ww))


class Form:
    def __init__(self, X, Y, ls, hyper, omega, phase, weights, eps, out):
        self.models = [Model(X, Y[:, b], ls[b], hyper[b, 0], hyper[b, 1], hyper[b, 2], omega[b], phase[b], weights[b], eps[b])
                       for b in range(len(ls))]
        self.out_mean, self.out_scale = out

    def all(self, Q):
        return np.stack([self.out_mean[b] + self.out_scale[b] * m.all(Q) for b, m in enumerate(self.models)], axis=1)

    def step(self, Qs):
        return np.stack([self.out_mean[b] + self.out_scale[b] * m.step(Qs) for b, m in enumerate(self.models)], axis=1)

    def rollout(self, x0, U, lin, coord, in_shift, in_scale):
        traj = [x0]
        for u in U:
            x = traj[-1]
            q = np.concatenate([x, np.broadcast_to(u, (len(x), len(u)))], axis=1)
            nxt = x + mm(q, lin.T)
            nxt[:, coord] += self.step((q - in_shift) / in_scale)
            traj.append(nxt)
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
    for i, (name, N, D, F, S, B, nx, H) in enumerate(CASES):
        rng = np.random.RandomState(1900 + i)
        # distinct per model: length-scales, signal variance, noise
        ls = np.stack([1.2 * (1.0 + 0.1 * np.arange(D)) * (1.0 + 0.15 * b) for b in range(B)])
        hyper = np.stack([[0.8 + 0.1 * b, 0.05 * (1 + b), ALPHA] for b in range(B)])
        in_shift, in_scale, outs = np.zeros(D), np.ones(D), np.stack([np.zeros(B), np.ones(B)])
        coord = np.arange(B)
        if name == "csv":
            raw, Yraw, Xq_raw = csv["X10"][:N], csv["Y6"][:N], csv["Xq10"][:MQ]
            # the scalers a trainer puts in front of and behind the models (population variance)
            in_shift, in_scale = raw.mean(axis=0), raw.std(axis=0)
            in_scale = np.where(in_scale > 1e-12, in_scale, 1.0)
            outs = np.stack([Yraw.mean(axis=0), Yraw.std(axis=0)])
            X, Y, Xq = (raw - in_shift) / in_scale, (Yraw - outs[0]) / outs[1], (Xq_raw - in_shift) / in_scale
            # (the models normalise their targets once more, normalize_y=True: a shifted, stretched copy keeps that visible)
            Y = 0.3 + 1.7 * Y
            outs = np.stack([outs[0] - 0.3 * outs[1] / 1.7, outs[1] / 1.7])
            ls = np.stack([2.0 * (1.0 + 0.05 * np.arange(D)) * (1.0 + 0.1 * b) for b in range(B)])
            dt = 0.02
            lin = np.zeros((nx, D))
            lin[0:3, 3:6] = dt * np.eye(3)                       # the double integrator of GPTrainer._nominal_dynamics
            lin[3:6, 6:9] = dt * np.eye(3)
            x0 = np.repeat(raw[17:18, :nx], S, axis=0)
            U = raw[40:40 + H, nx:].copy()
        else:
            X = rng.standard_normal((N, D))
            Wm = rng.standard_normal((D, B))
            Y = np.sin(mm(X, Wm)) + 0.5 * X[:, :1] + 0.1 * rng.standard_normal((N, B)) + np.arange(1, B + 1)
            Xq = rng.standard_normal((MQ, D))
            if name == "gap":
                coord = np.array(GAP_COORD)
            if H:
                lin = 0.1 * rng.standard_normal((nx, D))
                x0 = 0.5 * rng.standard_normal((S, nx))
                U = 0.5 * rng.standard_normal((H, D - nx))
                # the models' targets sit near 1 .. B: take most of that out again so that the state stays where the data is
                outs = np.stack([-0.1 * np.arange(1, B + 1), np.full(B, 0.1)])
        omega, phase, weights, eps = draw(rng, N, D, F, S, ls, hyper[:, 1] + ALPHA)
        # the two large arrays are kept in single precision, which keeps the file under the repository's size limit: the path
        # sets are built from the rounded numbers, widened again
        weights, eps = (a.astype(np.float32).astype(np.float64) for a in (weights, eps))
        Xs = np.concatenate([Xq, rng.standard_normal((max(S - MQ, 0), D))])[:S]
        form = Form(X, Y, ls, hyper, omega, phase, weights, eps, outs)
        arrays = {"X": X, "Y": Y, "Xq": Xq, "ls": ls, "hyper": hyper, "omega": omega, "phase": phase, "weights": weights,
                  "eps": eps, "Xs": Xs, "out": outs, "all": form.all(Xq), "step": form.step(Xs)}
        if H:
            arrays.update({"x0": x0, "U": U, "lin": lin, "coord": coord.astype(np.float64), "in": np.stack([in_shift, in_scale]),
                           "traj": form.rollout(x0, U, lin, coord, in_shift, in_scale)})
        for k, v in arrays.items():
            out[f"{name}_{k}"] = np.ascontiguousarray(v, dtype=np.float32 if k in ("weights", "eps") else np.float64)
        print(f"case {name}: N={N} D={D} F={F} S={S} B={B} nx={nx} H={H}  max|all| {np.abs(arrays['all']).max():.3g}"
              + (f"  max|traj| {np.abs(arrays['traj']).max():.3g}" if H else ""))
    return out


if __name__ == "__main__":
    save_npz(OUT, build())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
