"""Per-output ARD GP trainer / loader — the reference's alternative offline trainer on MI355X.

`GPTrainer.load_training_data` mirrors `src/px4/gp_trainer.py:49-119` (flight_data_*.npz -> [state, control] rows and
double-integrator residuals); `GPTrainer.train_gp_models` mirrors `src/px4/gp_trainer.py:121-205`: 80/20 split with seed 42,
one independent GP per residual component, z-scored inputs and target,
`C(1, fixed) * RBF(ls in R^D, bounds 0.1..10) + WhiteKernel(0.01, 1e-5..10)`, `alpha=1e-6`,
3 optimiser restarts.  `PreTrainedGP.predict_residual` mirrors `src/px4/pretrained_gp.py:52-98`
(returns the *standard deviation*, un-scaled by the target scaler), plus a batched variant.
The pickle layout `{'gp_models','scalers_X','scalers_y','training_stats','model_name',
'creation_time'}` is the reference's (`gp_trainer.py:214-221`).
"""
from __future__ import annotations

import os
import pickle
import time
from datetime import datetime

import numpy as np

from .gpr import GaussianProcessRegressor
from .kernels import RBF, ConstantKernel, WhiteKernel
from .sparse import SparseGP

OUTPUT_NAMES = ["x_residual", "y_residual", "z_residual", "vx_residual", "vy_residual", "vz_residual"]


class StandardScaler:
    """z-scoring with the population variance, as the reference gets it from scikit-learn 1.7.2
    (`gp_trainer.py:152-156` -> `sklearn/preprocessing/_data.py` StandardScaler.partial_fit): the variance is the
    corrected two-pass form of `_incremental_mean_and_var`, and a feature counts as constant (scale 1) when its variance
    is not above `n eps var + (n mean eps)^2` (`_is_constant_feature`) - NOT when its std is below 10 eps: the yaw-rate
    column of the flight CSVs has a std of 1e-21 and is scaled to unit variance like every other column."""

    def fit(self, A):
        A = np.asarray(A, dtype=np.float64)
        n = A.shape[0]
        self.mean_ = A.sum(axis=0) / n
        temp = A - self.mean_
        correction = temp.sum(axis=0)
        self.var_ = ((temp ** 2).sum(axis=0) - correction ** 2 / n) / n
        eps = np.finfo(np.float64).eps
        constant = self.var_ <= n * eps * self.var_ + (n * self.mean_ * eps) ** 2
        scale = np.sqrt(self.var_)
        self.scale_ = np.where(constant | (scale == 0.0), 1.0, scale)
        return self

    def transform(self, A):
        return (np.asarray(A, dtype=np.float64) - self.mean_) / self.scale_

    def fit_transform(self, A):
        return self.fit(A).transform(A)

    def inverse_transform(self, A):
        return np.asarray(A, dtype=np.float64) * self.scale_ + self.mean_


def _as_scaler(obj):
    """This package's `StandardScaler` from any object carrying `mean_` and `scale_` (e.g. the scikit-learn
    scalers inside a pickle written by the reference's `gp_trainer.py:214-221`)."""
    if isinstance(obj, StandardScaler):
        return obj
    s = StandardScaler()
    s.mean_ = np.asarray(obj.mean_, dtype=np.float64).copy()
    s.scale_ = np.asarray(obj.scale_, dtype=np.float64).copy()
    return s


def train_test_split(X, y, test_size=0.2, random_state=42):
    """Shuffled split: permutation from RandomState(seed); the first ceil(test_size * n) indices are
    the test set, the rest the training set (the ShuffleSplit rule the reference relies on)."""
    n = len(X)
    n_test = int(np.ceil(test_size * n))
    n_train = int(np.floor((1.0 - test_size) * n))
    perm = np.random.RandomState(random_state).permutation(n)
    te, tr = perm[:n_test], perm[n_test:n_test + n_train]
    return X[tr], X[te], y[tr], y[te]


def _r2(y_true, y_pred):
    ss_res = np.sum((y_true - y_pred) ** 2)
    ss_tot = np.sum((y_true - np.mean(y_true)) ** 2)
    return 1.0 - ss_res / ss_tot if ss_tot > 0 else 0.0


def hessian_to_raw(H_scaled, scale_x, scale_y):
    """The Hessian of a model behind scalers, in raw units.  The model reads z = (x - shift) / scale_x and its output goes
    through y = mean + scale_y f, so with H_scaled[..., d, e] = d2 f / dz_d dz_e:

        H_raw[..., d, e] = scale_y / (scale_x[d] scale_x[e]) * H_scaled[..., d, e]

    H_scaled (..., D, D), scale_x (D,), scale_y a scalar.  Both mirror entries get the same factor in the same order of
    operations, so a bit-symmetric input stays bit-symmetric."""
    H = np.asarray(H_scaled, dtype=np.float64)
    sx = np.asarray(scale_x, dtype=np.float64).ravel()
    if H.ndim < 2 or H.shape[-1] != sx.size or H.shape[-2] != sx.size:
        raise ValueError(f"H_scaled must be (..., {sx.size}, {sx.size})")
    return float(scale_y) * H / (sx[:, None] * sx[None, :])


class GPTrainer:
    def __init__(self, data_dir="gp_data", model_dir="gp_models", device=None):
        self.data_dir = data_dir
        self.model_dir = model_dir
        self.device = device
        self.gp_models, self.scalers_X, self.scalers_y, self.training_stats = {}, {}, {}, {}

    def load_training_data(self, max_samples=None):
        """`flight_data_*.npz` files of `data_dir` -> (X (n, 10) = [state_prev | control], y (n, 6) = residuals against the
        double-integrator nominal model).  Mirrors `src/px4/gp_trainer.py:49-102`: every file carries `states_prev`
        (n, 6), `controls` (n, 4), `states_next` (n, 6), `dt_values` (n,); residual = next - nominal(prev, control, dt);
        `max_samples` draws rows without replacement from the GLOBAL NumPy RNG (`np.random.choice`, :94-97), as the
        reference does.  The files are visited in sorted order (the reference's unsorted glob makes the row order
        depend on the file system)."""
        import glob
        data_files = sorted(glob.glob(os.path.join(self.data_dir, "flight_data_*.npz")))
        if not data_files:
            raise FileNotFoundError(f"No training data found in {self.data_dir}")
        all_X, all_y = [], []
        for data_file in data_files:
            with np.load(data_file) as data:
                states_prev = np.asarray(data["states_prev"], dtype=np.float64)
                controls = np.asarray(data["controls"], dtype=np.float64)
                states_next = np.asarray(data["states_next"], dtype=np.float64)
                dt_values = np.asarray(data["dt_values"], dtype=np.float64).reshape(-1)
            n = len(states_prev)            # (the reference walks range(len(states_prev)))
            nominal = self._nominal_dynamics(states_prev[:n], controls[:n], dt_values[:n, None])
            all_X.append(np.concatenate([states_prev[:n], controls[:n]], axis=1))
            all_y.append(states_next[:n] - nominal)
        X, y = np.concatenate(all_X, axis=0), np.concatenate(all_y, axis=0)
        if max_samples and len(X) > max_samples:
            indices = np.random.choice(len(X), max_samples, replace=False)
            X, y = X[indices], y[indices]
        return X, y

    @staticmethod
    def _nominal_dynamics(state, control, dt):
        """Double integrator (`gp_trainer.py:104-119`): pos + vel dt, vel + accel dt; rows at once (the same fp64
        operations per element as the reference's per-row form)."""
        state, control = np.asarray(state, dtype=np.float64), np.asarray(control, dtype=np.float64)
        pos, vel, accel = state[..., :3], state[..., 3:6], control[..., :3]
        return np.concatenate([pos + vel * dt, vel + accel * dt], axis=-1)

    def train_gp_models(self, X, y, test_size=0.2, n_restarts_optimizer=3, optimizer="fmin_l_bfgs_b", batched=True):
        """batched=True (default): the per-output models share X, so they are trained together — one fused
        launch chain per optimiser evaluation (`BatchedARDGP`); batched=False trains them one by one as the
        reference does."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        X_tr, X_te, y_tr, y_te = train_test_split(X, y, test_size=test_size, random_state=42)
        results = {}
        names = [n for i, n in enumerate(OUTPUT_NAMES[: y.shape[1]]) if np.std(y_tr[:, i]) >= 1e-6]
        if batched and 2 <= len(names) <= 8 and optimizer == "fmin_l_bfgs_b":
            from .batched import BatchedARDGP
            idx = [OUTPUT_NAMES.index(n) for n in names]
            sx = StandardScaler().fit(X_tr)
            sys_ = [StandardScaler().fit(y_tr[:, i].reshape(-1, 1)) for i in idx]
            Ys = np.column_stack([s_.transform(y_tr[:, i].reshape(-1, 1)).ravel() for s_, i in zip(sys_, idx)])
            bg = BatchedARDGP(length_scale=1.0, length_scale_bounds=(0.1, 10.0), noise_level=0.01,
                              noise_level_bounds=(1e-5, 1e1), alpha=1e-6, normalize_y=False, optimizer=optimizer,
                              n_restarts_optimizer=n_restarts_optimizer, device=self.device).fit(sx.transform(X_tr), Ys)
            pred_s = bg.predict(sx.transform(X_te))
            for j, (name, i) in enumerate(zip(names, idx)):
                gp, sy = bg.models[j], sys_[j]
                pred = sy.inverse_transform(pred_s[:, j].reshape(-1, 1)).flatten()
                mse = float(np.mean((y_te[:, i] - pred) ** 2))
                self.gp_models[name], self.scalers_X[name], self.scalers_y[name] = gp, sx, sy
                results[name] = {"mse": mse, "rmse": float(np.sqrt(mse)), "r2": float(_r2(y_te[:, i], pred)),
                                 "kernel": str(gp.kernel_), "log_marginal_likelihood": gp.log_marginal_likelihood()}
            self.training_stats = results
            return results
        for i, name in enumerate(OUTPUT_NAMES[: y.shape[1]]):
            yi_tr, yi_te = y_tr[:, i], y_te[:, i]
            if np.std(yi_tr) < 1e-6:          # gp_trainer.py:148-150
                continue
            sx, sy = StandardScaler(), StandardScaler()
            Xs = sx.fit_transform(X_tr)
            ys = sy.fit_transform(yi_tr.reshape(-1, 1)).flatten()
            kernel = (ConstantKernel(1.0, constant_value_bounds="fixed")
                      * RBF(length_scale=[1.0] * X.shape[1], length_scale_bounds=(0.1, 10.0))
                      + WhiteKernel(noise_level=0.01, noise_level_bounds=(1e-5, 1e1)))
            gp = GaussianProcessRegressor(kernel=kernel, n_restarts_optimizer=n_restarts_optimizer, alpha=1e-6,
                                          normalize_y=False, optimizer=optimizer, device=self.device)
            gp.fit(Xs, ys)
            pred = sy.inverse_transform(gp.predict(sx.transform(X_te)).reshape(-1, 1)).flatten()
            mse = float(np.mean((yi_te - pred) ** 2))
            self.gp_models[name], self.scalers_X[name], self.scalers_y[name] = gp, sx, sy
            results[name] = {"mse": mse, "rmse": float(np.sqrt(mse)), "r2": float(_r2(yi_te, pred)),
                             "kernel": str(gp.kernel_), "log_marginal_likelihood": gp.log_marginal_likelihood()}
        self.training_stats = results
        return results

    def sparsify(self, X, y, inducing, selection="greedy", train=False, approximation="dtc", **train_kw):
        """Replaces every trained exact model by a sparse one that has seen ALL rows of X (n, 10), y (n, 6) - the rows a
        `max_samples` cap (`load_training_data`, `src/px4/gp_trainer.py:95-96`) had thrown away included: per model
        `SparseGP.from_exact(model, inducing, selection=...)` on that model's own (scaled) training inputs, then
        `partial_fit` on all rows scaled with the stored scalers and, with train=True, `SparseGP.train(rows, **train_kw)`.
        `save_models()` then writes a file that `PreTrainedGP` loads and serves through `BatchedSparseGP`: all models in one
        call.  Models that are sparse already are left alone.  approximation: "dtc" or "fitc", as `SparseGP` takes it; with
        "fitc" and train=True the model is trained as DTC (the FITC likelihood has no gradient here) and the FITC model is then
        built from the trained kernel and inducing inputs and given all rows."""
        from .sparse import check_approximation
        check_approximation(approximation)
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        for name, model in list(self.gp_models.items()):
            if isinstance(model, SparseGP):
                continue
            i = OUTPUT_NAMES.index(name)
            Xs = self.scalers_X[name].transform(X)
            ys = self.scalers_y[name].transform(y[:, i].reshape(-1, 1)).ravel()
            sp = SparseGP.from_exact(model, inducing, selection=selection, approximation="dtc" if train else approximation)
            if train:
                sp.train(Xs, ys, **train_kw)
                if approximation == "fitc":
                    sp = SparseGP(sp.kernel_, sp.inducing_, alpha=sp.alpha, jitter_uu=sp.jitter_uu, y_mean=sp.y_mean, y_std=sp.y_std,
                                  device=sp.device, approximation="fitc").partial_fit(Xs, ys)
            else:
                sp.partial_fit(Xs, ys)
            self.gp_models[name] = sp
        return self

    def save_models(self, model_name=None):
        if model_name is None:
            model_name = f"gp_model_{datetime.now().strftime('%Y%m%d_%H%M%S')}"
        os.makedirs(self.model_dir, exist_ok=True)
        path = os.path.join(self.model_dir, f"{model_name}.pkl")
        with open(path, "wb") as f:
            pickle.dump({"gp_models": self.gp_models, "scalers_X": self.scalers_X, "scalers_y": self.scalers_y,
                         "training_stats": self.training_stats, "model_name": model_name,
                         "creation_time": time.time()}, f)
        return path

    def load_models(self, model_path):
        with open(model_path, "rb") as f:
            d = pickle.load(f)
        self.gp_models = {n: (m if isinstance(m, (GaussianProcessRegressor, SparseGP))
                              else GaussianProcessRegressor.from_sklearn(m, device=self.device))
                          for n, m in d["gp_models"].items()}
        self.scalers_X = {n: _as_scaler(v) for n, v in d["scalers_X"].items()}
        self.scalers_y = {n: _as_scaler(v) for n, v in d["scalers_y"].items()}
        self.training_stats = d["training_stats"]


class PreTrainedGP:
    def __init__(self, model_path):
        self.model_path = model_path
        self.gp_models, self.scalers_X, self.scalers_y, self.training_stats = {}, {}, {}, {}
        self.is_loaded = False
        self._axis_paths = None     # sample_rollouts: (key, BatchedPosteriorPaths) of the loaded models
        self.load_models()

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_axis_paths"] = None    # device buffers: drawn again on the first `sample_rollouts` after unpickling
        return st

    def load_models(self):
        if not os.path.exists(self.model_path):
            print(f"GP model file not found: {self.model_path}")
            return False
        try:
            with open(self.model_path, "rb") as f:
                d = pickle.load(f)
            return self.load_dict(d)
        except Exception as e:  # noqa: BLE001
            print(f"Failed to load GP models: {e}")
            return False

    def load_dict(self, d, device=None):
        """Install the content of a model file.  The file may have been written by this package's `GPTrainer` or
        by the reference's (`src/px4/gp_trainer.py:214-221`: scikit-learn regressors and scikit-learn
        `StandardScaler`s): foreign regressors are ingested with `GaussianProcessRegressor.from_sklearn`
        (X_train_, alpha_, L_, kernel_ and the target normalisation taken as they are), and any object carrying
        `mean_` / `scale_` serves as a scaler.  A `SparseGP` (`GPTrainer.sparsify`) is kept as it is: its statistics are
        imported on the device at the first prediction.  A component that cannot be converted is dropped (its prediction is
        then the reference's (0, 1e6) fallback, `pretrained_gp.py:93-96`)."""
        models, sxs, sys_ = {}, {}, {}
        self._axis_paths = None
        for name, m in d["gp_models"].items():
            try:
                if not isinstance(m, (GaussianProcessRegressor, SparseGP)):
                    m = GaussianProcessRegressor.from_sklearn(m, device=device)
                models[name] = m
                sxs[name] = _as_scaler(d["scalers_X"][name])
                sys_[name] = _as_scaler(d["scalers_y"][name])
            except Exception as e:  # noqa: BLE001
                print(f"GP model {name} could not be loaded: {e}")
                models.pop(name, None)
        if d["gp_models"] and not models:
            # nothing survived the conversion: as in the reference, where a failed load leaves `is_loaded` False
            # (`pretrained_gp.py:34-50`) and every prediction is the (0, 1e6) fallback
            self.gp_models, self.scalers_X, self.scalers_y, self.training_stats = {}, {}, {}, {}
            self._fused_bg = None
            self.is_loaded = False
            return False
        self.gp_models, self.scalers_X, self.scalers_y = models, sxs, sys_
        self.training_stats = d.get("training_stats", {})
        self._fused_bg = None
        self.is_loaded = True
        return True

    def predict_residual(self, state, control):
        """One query -> (mean (6,), std (6,)); missing / failing components -> (0, 1e6).  Never raises
        (`pretrained_gp.py:52-98`: the control loop calls this every step)."""
        try:
            mean, std = self.predict_residual_batch(
                np.concatenate([np.asarray(state, float)[:6], np.asarray(control, float)[:4]]).reshape(1, -1))
            return mean[0], std[0]
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros(6), np.ones(6) * 1e6

    def _fused(self):
        """All loaded models share the input scaler and training inputs (they do when written by `GPTrainer`):
        evaluate their means with one fused launch.  Sparse models (`GPTrainer.sparsify`): single-output `SparseGP`s with
        equal m, D and input scalers are served through `BatchedSparseGP`, all of them in one call."""
        if getattr(self, "_fused_bg", None) is None:
            self._fused_bg = False
            try:
                names = [n for n in OUTPUT_NAMES if n in self.gp_models]
                ms = [self.gp_models[n] for n in names]
                if 2 <= len(names) <= 8 and self._one_input_scaler(names):
                    if all(isinstance(m, SparseGP) for m in ms):
                        if all(m.n_outputs_ == 1 and m.inducing_.shape == ms[0].inducing_.shape for m in ms):
                            from .sparse_batch import BatchedSparseGP
                            self._fused_bg = (BatchedSparseGP(ms), names)
                    else:
                        x0 = getattr(ms[0], "X_train_", None)
                        if x0 is not None and all(
                                getattr(m, "X_train_", np.empty(0)).shape == x0.shape and np.array_equal(m.X_train_, x0) and
                                getattr(m, "_yn", np.empty((0, 0))).shape[1:] == (1,) for m in ms):
                            from .batched import BatchedARDGP
                            bg = BatchedARDGP(optimizer=None)
                            bg.models = ms
                            self._fused_bg = (bg, names)
            except Exception as e:  # noqa: BLE001 - never into the control loop: the per-model path below still serves
                print(f"fused per-axis prediction unavailable: {e}")
        return self._fused_bg

    @property
    def approximations_(self):
        """{output name: "dtc" or "fitc"} for the sparse models of the file (`GPTrainer.sparsify(approximation=...)`); exact
        models are not listed."""
        return {n: m.approximation_ for n, m in self.gp_models.items() if isinstance(m, SparseGP)}

    def _one_input_scaler(self, names):
        sx0 = self.scalers_X[names[0]]
        return all(np.array_equal(self.scalers_X[n].mean_, sx0.mean_) and np.array_equal(self.scalers_X[n].scale_, sx0.scale_)
                   for n in names)

    def _serve(self, X, fused_call, model_call, put, fallback):
        """The skeleton of the three batch surfaces: the fused object (`_fused`) serves all its models in one call on the rows
        scaled with their shared input scaler (`_serve_fused`); whatever that left - no fused object, a failed call, a
        component `put` refused - is served model by model with the model's own scaler (`_serve_models`); a component whose
        own call fails gets `fallback(i)`.  `fused_call(bg, Xs)` returns a tuple of arrays with the models along axis 1 (None:
        not computed), `model_call(m, Xs)` the same tuple for one model; `put(i, name, sx, result)` undoes the scalers and
        fills component i of the caller's arrays, or raises.  Failures are printed, never raised."""
        done, _ = self._serve_fused(X, fused_call, put)
        self._serve_models(X, model_call, put, fallback, done)

    def _serve_fused(self, X, fused_call, put):
        """The fused stage of `_serve`: (the names it filled, whether it failed part-way or altogether)."""
        done = set()
        fused = self._fused()
        if fused:
            bg, names = fused
            try:
                sx = self.scalers_X[names[0]]
                out = fused_call(bg, sx.transform(X))
                for j, n in enumerate(names):
                    put(OUTPUT_NAMES.index(n), n, sx, tuple(None if o is None else o[:, j] for o in out))
                    done.add(n)
            except Exception as e:  # noqa: BLE001 - the per-model stage still serves
                print(f"GP prediction failed: {e}")
                return done, True
        return done, False

    def _serve_models(self, X, model_call, put, fallback, done):
        """The per-model stage of `_serve`, for every loaded model not in `done`."""
        for i, name in enumerate(OUTPUT_NAMES):
            if name not in self.gp_models or name in done:
                continue
            try:
                sx = self.scalers_X[name]
                put(i, name, sx, model_call(self.gp_models[name], sx.transform(X)))
            except Exception as e:  # noqa: BLE001
                print(f"GP prediction failed for {name}: {e}")
                fallback(i)

    def predict_residual_batch(self, X, return_std=True):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        mean, std = np.zeros((len(X), 6)), np.full((len(X), 6), 1e6)
        if not self.is_loaded:
            return mean, std

        def put(i, name, sx, result):
            m, s = result
            sy = self.scalers_y[name]
            mean[:, i] = sy.inverse_transform(m.reshape(-1, 1)).ravel()
            if s is not None:
                std[:, i] = np.abs(s * sy.scale_[0])

        def fallback(i):
            mean[:, i], std[:, i] = 0.0, 1e6

        # models written by `GPTrainer` share scaler and inputs: all of them in one call (<= 32 rows: one C call and two
        # launches for means and stds, `gpk_predict_host_multi`; larger batches: one fused mean launch).  The models' own
        # calls always compute the stds; they are handed back whenever no fused object stood in front of them.
        def fused_call(bg, Xs):
            out = bg.predict(Xs, return_std=return_std)
            return out if return_std else (out, None)

        done, failed = self._serve_fused(X, fused_call, put)
        if failed:
            # Special to this surface, kept as it has always behaved: a fused stage that fails keeps nothing of what it had
            # filled, and without return_std the call ends here with zeros - the models' own calls are not tried.
            mean[:], std[:] = 0.0, 1e6
            if not return_std:
                return mean, None
            done = set()
        self._serve_models(X, lambda m, Xs: m.predict(Xs, return_std=True), put, fallback, done)
        return mean, (std if return_std or not self._fused() else None)

    # ---- input gradients: the first-order terms of the per-axis models in raw units ---------------------------------
    def predict_residual_jacobian_batch(self, X, return_std=False):
        """Residual means of a batch of raw [state(6), control(4)] rows and their Jacobians with respect to those raw
        inputs - what an MPC linearises with (quadrotor_gp_mpc/quadrotor_gp_mpc/mpc_controller.py:318) - and, with
        return_std=True, the standard deviations `predict_residual_batch` returns and their gradients:
        (mean (M, 6), J (M, 6, 10)[, std (M, 6), dstd (M, 6, 10)]).  With z = (x - sx.mean_) / sx.scale_, mu_b / var_b model
        b's posterior on the scaled inputs and sy_b its target scaler:

            J[m, b, d]    = sy_b.scale_ / sx.scale_[d] * d mu_b / d z_d
            dstd[m, b, d] = |sy_b.scale_| / sx.scale_[d] * (d var_b / d z_d) / (2 sigma_b)        (0 where sigma_b = 0)

        Models that share inputs and scaler (those `GPTrainer` writes): ONE call for all of them
        (`BatchedARDGP.predict_jacobian`; up to 32 rows one launch for means + Jacobians, three with the variances); otherwise
        one `predict_jacobian` per model with its own scalers.  The reference has no counterpart: a caller would difference
        `pretrained_gp.py:52-98`.  Missing or failing components: mean 0, J 0, std 1e6, dstd 0.  Never raises."""
        try:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            M = len(X)
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            X, M = None, 1
        mean, J = np.zeros((M, 6)), np.zeros((M, 6, 10))
        std, dstd = np.full((M, 6), 1e6), np.zeros((M, 6, 10))

        def put(i, name, sx, result):
            mu, dmu, var, dvar = (result + (None, None))[:4]
            sy = self.scalers_y[name]
            scale_y = float(np.ravel(sy.scale_)[0])
            m_i = sy.inverse_transform(np.asarray(mu, dtype=np.float64).reshape(-1, 1)).ravel()
            J_i = scale_y * np.asarray(dmu, dtype=np.float64).reshape(M, -1) / sx.scale_[None, :]
            if return_std:
                sig = np.sqrt(np.asarray(var, dtype=np.float64).reshape(M))
                pos = sig > 0.0
                g = np.zeros((M, J_i.shape[1]))
                g[pos] = np.asarray(dvar, dtype=np.float64).reshape(M, -1)[pos] / (2.0 * sig[pos, None])
                s_i, ds_i = np.abs(sig * scale_y), abs(scale_y) * g / sx.scale_[None, :]
                if not (np.isfinite(s_i).all() and np.isfinite(ds_i).all()):
                    raise FloatingPointError("non-finite standard deviation or gradient")
            if not (np.isfinite(m_i).all() and np.isfinite(J_i).all()):
                raise FloatingPointError("non-finite mean or Jacobian")
            mean[:, i], J[:, i, :] = m_i, J_i
            if return_std:
                std[:, i], dstd[:, i, :] = s_i, ds_i

        def fallback(i):
            mean[:, i], J[:, i], std[:, i], dstd[:, i] = 0.0, 0.0, 1e6, 0.0

        if X is not None and self.is_loaded and X.shape[1] == 10:
            self._serve(X, lambda bg, Xs: tuple(bg.predict_jacobian(Xs, return_var=return_std)),
                        lambda m, Xs: tuple(m.predict_jacobian(Xs, return_var=return_std)), put, fallback)
        if return_std:
            return mean, J, std, dstd
        return mean, J

    # ---- joint posterior along a batch of rows: covariances and draws in raw units ---------------------------------------
    FALLBACK_VAR = 1e12        # the square of the 1e6 this class reports as the std of a missing component

    def _residual_cov(self, X):
        """(mean (M, 6), cov (M, M, 6), served (6,) bool) of `predict_residual_cov_batch`."""
        try:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            M = len(X)
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            X, M = None, 1
        mean = np.zeros((M, 6))
        cov = np.repeat((self.FALLBACK_VAR * np.eye(M))[:, :, None], 6, axis=2)
        served = np.zeros(6, dtype=bool)

        def put(i, name, sx, result):
            mu, sig = result
            sy = self.scalers_y[name]
            m_i = sy.inverse_transform(np.asarray(mu, dtype=np.float64).reshape(-1, 1)).ravel()
            c_i = float(np.ravel(sy.scale_)[0]) ** 2 * np.asarray(sig, dtype=np.float64).reshape(M, M)
            if not (np.isfinite(m_i).all() and np.isfinite(c_i).all()):
                raise FloatingPointError("non-finite mean or covariance")
            mean[:, i], cov[:, :, i], served[i] = m_i, c_i, True

        def fallback(i):
            mean[:, i], cov[:, :, i], served[i] = 0.0, self.FALLBACK_VAR * np.eye(M), False

        def fused_call(bg, Xs):     # (cov (M, M, B): the models along axis 1 for `_serve`)
            mu, sig = bg.predict(Xs, return_cov=True)
            return mu, np.moveaxis(sig, 2, 1)

        if X is not None and self.is_loaded:
            self._serve(X, fused_call, lambda m, Xs: m.predict(Xs, return_cov=True), put, fallback)
        return mean, cov, served

    def predict_residual_cov_batch(self, X):
        """Joint posterior of the six residuals over a batch of raw [state(6), control(4)] rows - a consistent residual
        trajectory per axis along the horizon: (mean (M, 6), cov (M, M, 6)) in raw units, cov[..., i] = sy_i.scale_^2 Sigma_i
        with Sigma_i model i's posterior covariance on the scaled inputs (its WhiteKernel level on the diagonal, not clipped).
        Models that share inputs and scaler (those `GPTrainer` writes): ONE call for all of them
        (`BatchedARDGP.predict(return_cov=True)`; up to 32 rows two launches and one synchronisation); otherwise one
        `predict(return_cov=True)` per model with its own scalers.  The reference has no counterpart: a caller would make
        six scikit-learn `predict(return_cov=True)` calls around `pretrained_gp.py:52-98`.  Missing or failing components, or
        nothing loaded: mean 0, cov[..., i] = 1e12 I.  Never raises."""
        mean, cov, _ = self._residual_cov(X)
        return mean, cov

    def sample_residuals(self, X, n_samples=1, random_state=0):
        """Draws from that joint posterior: (M, 6, n_samples) in raw units, through the Cholesky factor of each covariance
        (`gpr.cholesky_draws`).  One standard-normal block of shape (6, M, n_samples) is drawn whatever is loaded, so a
        component's draw does not depend on which others are present.  Missing or failing components: zeros.  Never raises."""
        from .gpr import cholesky_draws
        mean, cov, served = self._residual_cov(X)
        try:
            return cholesky_draws(mean, cov, n_samples, random_state, active=served)
        except Exception as e:  # noqa: BLE001
            print(f"GP sampling failed: {e}")
            return np.zeros((mean.shape[0], 6, int(n_samples)))

    def sample_rollouts(self, state, U_guess, dt, n_rollouts=64, n_features=1024, random_state=0, return_jacobian=False):
        """`n_rollouts` closed-loop rollouts under the loaded models' own uncertainty, in raw units: rollout r follows ONE
        posterior function draw of every per-axis model along the whole horizon, stage k + 1 evaluated at the state its
        sampled residuals of stage k produced,

            x_{k+1} = x_k + dt [v_k, a_k] + sum_i e_i (sy_i.mean_ + sy_i.scale_ f_{i,r}(([x_k, u_k] - sx.mean_) / sx.scale_))

        in one call for the horizon (`BatchedPosteriorPaths.rollout` on the fused `BatchedARDGP`, or
        `BatchedSparsePosteriorPaths.rollout` on the fused `BatchedSparseGP` of a `sparsify`-written file; the shared input
        scaler and each model's target scaler).  state (6,); U_guess (4, N).  Returns (R, 6, N + 1), the layout
        `linearize_residuals` takes as X_guess.  A residual without a model leaves its coordinate nominal.  The path set
        (n_rollouts, n_features, random_state) is drawn once and cached on the object until `load_dict` - or until a sparse
        model takes rows or is retrained (a path set is a snapshot) - the same functions from call to call.  Not loaded, models
        that cannot be fused into a batch (a single model, different inputs or scalers), or any failure: the reason is printed
        and the nominal trajectory is returned R times - it never raises into the control loop.

        return_jacobian=True: (X, J) in one call (`rollout(..., return_jacobian=True)` of the path set); X as above, with the
        same bits; J (R, N, 6, 10) in raw units: J[r, k, i] is the gradient of the SAMPLED residual of state coordinate i at
        stage k of rollout r w.r.t. [x_k, u_k] - the function that produced the rollout, not the posterior mean
        `linearize_residuals` linearises - and a coordinate without a model has a zero row.  With the `lin` of the nominal
        double integrator (`paths.nominal_rollouts`) the stage matrices of rollout r's closed loop are
        A_k = I + lin[:, :6] + J[r, k][:, :6] and B_k = lin[:, 6:] + J[r, k][:, 6:] (no gain / dt factor: J already is the
        derivative of the state increment).  Not loaded or failed: the nominal trajectory and a zero J."""
        from .paths import cached_path_set, nominal_rollouts, roll_paths
        U_guess = np.asarray(U_guess, dtype=float)
        state = np.asarray(state, dtype=float).reshape(-1)[:6]
        fallback, lin = nominal_rollouts(GPTrainer._nominal_dynamics, state, U_guess, dt, n_rollouts)
        if return_jacobian:
            fallback = (fallback, np.zeros((fallback.shape[0], U_guess.shape[1], 6, 10)))
        try:
            if not self.is_loaded:
                raise RuntimeError("no models are loaded")
            fused = self._fused()
            if not fused:
                raise RuntimeError("the loaded models are not served as one per-axis batch")
            bg, names = fused

            def target_scalers(paths):
                sys_ = [self.scalers_y[n] for n in names]
                paths.set_output_scaler([float(np.ravel(s.mean_)[0]) for s in sys_], [float(np.ravel(s.scale_)[0]) for s in sys_])

            paths = cached_path_set(self, "_axis_paths", bg, n_rollouts, n_features, random_state, finish=target_scalers)
            how = dict(coord=[OUTPUT_NAMES.index(n) for n in names], in_scaler=self.scalers_X[names[0]])
            if return_jacobian:
                traj, J = roll_paths(paths, state, U_guess, lin, return_jacobian=True, **how)
                if not (np.isfinite(traj).all() and np.isfinite(J).all()):
                    raise FloatingPointError("non-finite trajectory")
                return traj, J
            traj = roll_paths(paths, state, U_guess, lin, **how)
            if not np.isfinite(traj).all():
                raise FloatingPointError("non-finite trajectory")
            return traj
        except Exception as e:  # noqa: BLE001
            print(f"GP rollout sampling failed: {e}")
            return fallback

    def propagate_horizon(self, state, U_guess, dt, Sigma0=None, process_noise=None, order=1, method="linear"):
        """`SimpleQuadrotorGP.propagate_horizon` for the per-axis models, in raw units: the closed loop of the posterior MEANS
        and the state covariance the models' uncertainty induces along it, to first order,

            x_{k+1} = x_k + dt [v_k, a_k] + sum_i e_i mu_i(q_k),   Sigma_{k+1} = A_k Sigma_k A_k^T + sum_i var_i(q_k) e_i e_i^T + Q

        with mu_i = sy_i.mean_ + sy_i.scale_ m_i((q - sx.mean_) / sx.scale_), var_i its variance and A_k = I + lin[:, :6] + the
        rows d mu_i / d x.  Models that share inputs and scaler (those `GPTrainer` writes): ONE call for the horizon
        (`BatchedARDGP.propagate`: the shared input scaler and each model's target scaler; a file of sparse models:
        `BatchedSparseGP.propagate`, its one-call chain where `propagate_ok()` holds, else a host loop with one call for all
        models per stage); otherwise the same recursion model by
        model over `predict_residual_jacobian_batch`.  The variances are the latent functions' on both routes.  state (6,);
        U_guess (4, N) -> X (6, N + 1), Sigma (N + 1, 6, 6); U_guess (R, 4, N) -> (R, 6, N + 1), (R, N + 1, 6, 6).  A residual
        without a model leaves its coordinate nominal.  Not loaded, or any failure (printed): the nominal trajectory and
        Sigma_{k+1} = (I + lin_x) Sigma_k (I + lin_x)^T + Q - it never raises into the control loop.  order=2: x_{k+1} also takes
        tr(H_i Sigma_k) / 2 per model, H_i the state block of mu_i's raw Hessian (the batches' `propagate`; model by model over
        `predict_residual_hessian_batch`); any other order: ValueError.  method="moment": every stage's exact moments, all
        pairs of models included (`BatchedARDGP.propagate(method="moment")`; a file of sparse models: `BatchedSparseGP.propagate_moments`, one
        call for the horizon; models that share inputs and scaler only, anything else is a failure as above); ValueError with
        order=2."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.check_method(method, order)
        state, U, lin, nominal, single = _pg.horizon_inputs(GPTrainer._nominal_dynamics, state, U_guess, dt)
        try:
            if not self.is_loaded:
                raise RuntimeError("no models are loaded")
            fused = self._fused()
            if method == "moment" and not fused:
                raise RuntimeError("method='moment' needs models that share inputs and scaler")
            if fused:
                bg, names = fused
                sys_ = [self.scalers_y[n] for n in names]
                traj, Sigma = _pg.model_horizon(bg, state, U, lin, order=order, method=method,
                                                coord=[OUTPUT_NAMES.index(n) for n in names], in_scaler=self.scalers_X[names[0]],
                                                Sigma0=Sigma0, process_noise=process_noise,
                                                out_scaler=([float(np.ravel(s.mean_)[0]) for s in sys_],
                                                            [float(np.ravel(s.scale_)[0]) for s in sys_]))
            else:
                coord = [i for i, n in enumerate(OUTPUT_NAMES) if n in self.gp_models]
                x0, Uc, linc, S0, Q, R, H = _pg.check_horizon(state, U, lin, 6, 10, Sigma0, process_noise)
                # the noise level's share of every model's raw variance: the served variances carry it, the propagation
                # takes the latent function's
                lvl = np.array([(self.gp_models[OUTPUT_NAMES[i]].kernel_.components().noise or 0.0) *
                                (float(np.ravel(self.gp_models[OUTPUT_NAMES[i]]._y_train_std)[0]) *
                                 float(np.ravel(self.scalers_y[OUTPUT_NAMES[i]].scale_)[0])) ** 2 for i in coord])

                def stage(q):
                    mean, J, std, _ = self.predict_residual_jacobian_batch(q, return_std=True)
                    return mean[:, coord], J[:, coord, :], np.maximum(std[:, coord] ** 2 - lvl[None, :], 0.0)

                hess_stage = (lambda q: self.predict_residual_hessian_batch(q)[2][:, coord]) if order == 2 else None
                traj, Sigma, _ = _pg.host_loop(stage, coord, x0, Uc, linc, S0, Q, R, H, hess_stage)
            if not (np.isfinite(traj).all() and np.isfinite(Sigma).all()):
                raise FloatingPointError("non-finite trajectory or covariance")
            return _pg.horizon_layout(traj, Sigma, single)
        except Exception as e:  # noqa: BLE001
            print(f"GP horizon propagation failed: {e}")
            return _pg.horizon_layout(*_pg.nominal_horizon(nominal, lin, Sigma0, process_noise), single)

    def horizon_gradient(self, state, U_guess, dt, grad_traj, grad_Sigma=None, method="linear"):
        """`SimpleQuadrotorGP.horizon_gradient` for the per-axis models, in raw units: `propagate_horizon` (first order, Sigma0 =
        0, no process noise) with the gradient of a horizon cost with respect to the controls and the start state.  Models
        that share inputs and scaler: ONE call for the horizon (`BatchedARDGP.propagate_gradient`; a file of sparse models:
        `BatchedSparseGP.propagate_gradient`, its one-call chain where `propagate_ok()` holds).  Same shapes and results as
        `SimpleQuadrotorGP.horizon_gradient`.  Not loaded, models that do not share inputs and scaler, or any failure
        (printed): the nominal horizon and the sweep through the nominal dynamics - it never raises into the control loop.
        method="moment": the gradient through the exact moments of every stage (`BatchedARDGP.propagate_moments_gradient`, one
        call; a file of sparse models: `BatchedSparseGP.propagate_moments_gradient`, one call as well)."""
        from . import propagate as _pg
        state, U, lin, nominal, single = _pg.horizon_inputs(GPTrainer._nominal_dynamics, state, U_guess, dt)
        try:
            _pg.check_method(method)
            if not self.is_loaded:
                raise RuntimeError("no models are loaded")
            fused = self._fused()
            if not fused:
                raise RuntimeError("the models do not share inputs and scaler")
            bg, names = fused
            sys_ = [self.scalers_y[n] for n in names]
            kw = dict(coord=[OUTPUT_NAMES.index(n) for n in names], in_scaler=self.scalers_X[names[0]],
                      out_scaler=([float(np.ravel(s.mean_)[0]) for s in sys_], [float(np.ravel(s.scale_)[0]) for s in sys_]))
            if method == "moment":
                traj, Sigma, dU, dx0, _ = _pg.model_moments_gradient(bg, state, U, lin, grad_traj, grad_Sigma, **kw)
            else:
                traj, Sigma, dU, dx0, _ = bg.propagate_gradient(state, U, lin, grad_traj, grad_Sigma, route=_pg.wrapper_route(bg), **kw)
            if not all(np.isfinite(a).all() for a in (traj, Sigma, dU, dx0)):
                raise FloatingPointError("non-finite trajectory, covariance or gradient")
            return _pg.gradient_layout(traj, Sigma, dU, dx0, single)
        except Exception as e:  # noqa: BLE001
            print(f"GP horizon gradient failed: {e}")
            return _pg.nominal_gradient(nominal, lin, grad_traj, single)

    def predict_residual_jacobian(self, state, control):
        """One query -> (mean (6,), J (6, 10)), J = d mean / d [state(6), control(4)]; not loaded or failed: zeros."""
        try:
            row = np.concatenate([np.asarray(state, float)[:6], np.asarray(control, float)[:4]]).reshape(1, -1)
            mean, J = self.predict_residual_jacobian_batch(row)
            return mean[0], J[0]
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros(6), np.zeros((6, 10))

    # ---- second derivatives of the residual means in raw units ----------------------------------------------------------
    def predict_residual_hessian_batch(self, X):
        """Residual means of a batch of raw [state(6), control(4)] rows with their Jacobians and Hessians with respect to
        those raw inputs: (mean (M, 6), J (M, 6, 10), H (M, 6, 10, 10)); mean and J as `predict_residual_jacobian_batch`
        returns them, H by `hessian_to_raw` from model b's Hessian on the scaled inputs:

            H[m, b, d, e] = sy_b.scale_ / (sx.scale_[d] sx.scale_[e]) * d2 mu_b / dz_d dz_e

        Models that share inputs and scaler: ONE call for all of them (`BatchedARDGP.predict_hessian`, or
        `BatchedSparseGP.predict_hessian` for model files written by `sparsify`); otherwise one `predict_hessian` per model
        with its own scalers.  The reference has no counterpart.  Missing or failing components: zeros.  Never raises."""
        try:
            X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            M = len(X)
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            X, M = None, 1
        mean, J, H = np.zeros((M, 6)), np.zeros((M, 6, 10)), np.zeros((M, 6, 10, 10))

        def put(i, name, sx, result):
            mu, dmu, h = result
            sy = self.scalers_y[name]
            scale_y = float(np.ravel(sy.scale_)[0])
            m_i = sy.inverse_transform(np.asarray(mu, dtype=np.float64).reshape(-1, 1)).ravel()
            J_i = scale_y * np.asarray(dmu, dtype=np.float64).reshape(M, -1) / sx.scale_[None, :]
            H_i = hessian_to_raw(np.asarray(h, dtype=np.float64).reshape(M, 10, 10), sx.scale_, scale_y)
            if not (np.isfinite(m_i).all() and np.isfinite(J_i).all() and np.isfinite(H_i).all()):
                raise FloatingPointError("non-finite mean, Jacobian or Hessian")
            mean[:, i], J[:, i, :], H[:, i] = m_i, J_i, H_i

        def fallback(i):
            mean[:, i], J[:, i], H[:, i] = 0.0, 0.0, 0.0

        if X is not None and self.is_loaded and X.shape[1] == 10:
            self._serve(X, lambda bg, Xs: tuple(bg.predict_hessian(Xs)), lambda m, Xs: tuple(m.predict_hessian(Xs)), put,
                        fallback)
        return mean, J, H

    def predict_residual_hessian(self, state, control):
        """One query -> (mean (6,), J (6, 10), H (6, 10, 10)), the first and second derivatives of the residual means with
        respect to [state(6), control(4)]; not loaded or failed: zeros and a printed reason."""
        try:
            row = np.concatenate([np.asarray(state, float)[:6], np.asarray(control, float)[:4]]).reshape(1, -1)
            if not self.is_loaded:
                print("GP Hessian unavailable: no model loaded")
            mean, J, H = self.predict_residual_hessian_batch(row)
            return mean[0], J[0], H[0]
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros(6), np.zeros((6, 10)), np.zeros((6, 10, 10))

    def linearize_residuals(self, X_guess, U_guess, dt, gain=0.1, n_states=6):
        """`SimpleQuadrotorGP.linearize_gp_residuals` for the per-axis models: the frozen residual D (6, N) and its
        linearisation A (N, 6, 6), B (N, 6, 4) around the guess X_guess (6+, N+1), U_guess (4, N) - zero except rows 3:6 =
        gain / dt * J_k[3:6, :6] and gain / dt * J_k[3:6, 6:10] - from ONE call for the whole horizon; (R, ...) leading axis
        for R rollouts.  Not loaded or a failed prediction: zeros."""
        X_guess = np.asarray(X_guess, dtype=float)
        U_guess = np.asarray(U_guess, dtype=float)
        single = X_guess.ndim == 2
        if single:
            X_guess, U_guess = X_guess[None], U_guess[None]
        R, _, N = U_guess.shape
        D = np.zeros((R, n_states, N))
        A = np.zeros((R, N, n_states, 6))
        B = np.zeros((R, N, n_states, 4))
        if self.is_loaded:
            try:
                rows = np.concatenate([X_guess[:, :6, :N], U_guess[:, :4, :]], axis=1)    # (R, 10, N)
                rows = rows.transpose(0, 2, 1).reshape(R * N, -1)
                mean, J = self.predict_residual_jacobian_batch(rows)
                if n_states >= 6:
                    D[:, 3:6, :] = (gain * (mean / dt)[:, 3:6]).reshape(R, N, 3).transpose(0, 2, 1)
                    A[:, :, 3:6, :] = (gain / dt * J[:, 3:6, :6]).reshape(R, N, 3, 6)
                    B[:, :, 3:6, :] = (gain / dt * J[:, 3:6, 6:10]).reshape(R, N, 3, 4)
            except Exception as e:  # noqa: BLE001
                print(f"GP prediction failed: {e}")
                D[:], A[:], B[:] = 0.0, 0.0, 0.0
        if single:
            return D[0], A[0], B[0]
        return D, A, B

    def get_uncertainty(self, state, control):
        return float(np.mean(self.predict_residual(state, control)[1]))

    def get_stats(self):
        return {"is_loaded": self.is_loaded, "model_path": self.model_path,
                "available_models": list(self.gp_models.keys()), "training_stats": self.training_stats}
