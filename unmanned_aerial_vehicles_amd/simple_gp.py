"""`SimpleQuadrotorGP` — the model seam the GP-MPC ROS 2 nodes call, on MI355X.

Mirrors the public surface of the reference class (`src/px4/simple_gp.py:24-223`):
`add_training_data`, `train_gp`, `predict_residual`, `get_uncertainty`,
`predict_enhanced_dynamics`, `load_model`, `save_dataset`, `get_stats`, the attributes
`X_train`, `Y_train`, `gp_model`, `is_trained`, `training_count`, `prediction_count`, and the
"never raise into the control loop" fallbacks.  Added for the GPU: batched variants
(`predict_residual_batch`, `build_gp_residuals`) that replace the per-horizon-point Python
loop of `src/px4/mpc.py:1490-1506` by one fused kernel call.
"""
from __future__ import annotations

import os
import pickle
from collections import deque

import numpy as np

from .gpr import GaussianProcessRegressor
from .kernels import RBF, WhiteKernel

GPU_BACKEND_AVAILABLE = True  # the class fails loudly at train/predict time if the GPU is absent


class SimpleQuadrotorGP:
    """Multi-output GP on [x,y,z,vx,vy,vz, ax,ay,az,yaw_rate] -> 6 state residuals."""

    def __init__(self, max_data_points=1000, device=None, predict_dtype="float64"):
        self.max_data_points = max_data_points
        self.X_train = deque(maxlen=max_data_points)   # oldest rows are evicted (simple_gp.py:31-32)
        self.Y_train = deque(maxlen=max_data_points)
        self.gp_model = None
        self.is_trained = False
        self.training_count = 0
        self.prediction_count = 0
        self.device = device
        self.predict_dtype = predict_dtype
        self._paths = None          # sample_rollouts: (key, PosteriorPaths) of the current model

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_paths"] = None         # device buffers: drawn again on the first `sample_rollouts` after unpickling
        return st

    # ---- data ---------------------------------------------------------------------------------
    def _to_numpy(self):
        if len(self.X_train) == 0:
            return np.empty((0, 10)), np.empty((0, 6))
        return np.array(self.X_train), np.array(self.Y_train)

    def _nominal_dynamics(self, state, control, dt):
        """Double integrator: x+ = x + dt * [v, a]  (simple_gp.py:146-154)."""
        state = np.asarray(state, dtype=float)
        control = np.asarray(control, dtype=float)
        return state + dt * np.concatenate([state[3:6], control[:3]])

    def add_training_data(self, state, control, state_next, dt=0.02):
        """Quality filters of simple_gp.py:118-140: |v| <= 5, |a_cmd| <= 3, |residual| <= 2."""
        if len(state) < 6 or len(state_next) < 6:
            return
        state = np.asarray(state, dtype=float)
        control = np.asarray(control, dtype=float)
        if np.linalg.norm(state[3:6]) > 5.0 or np.linalg.norm(control[:3]) > 3.0:
            return
        residual = np.asarray(state_next, dtype=float) - self._nominal_dynamics(state, control, dt)
        if np.linalg.norm(residual) > 2.0:
            return
        self.X_train.append(np.concatenate([state[:6], control[:4]]))
        self.Y_train.append(residual.copy())

    def save_dataset(self, csv_path, include_header=True, overwrite=True):
        """16-column `%.18e` CSV (simple_gp.py:75-115)."""
        X, Y = self._to_numpy()
        if X.shape[0] == 0:
            print("No training data to save.")
            return
        from .data import save_dataset_csv
        save_dataset_csv(csv_path, X, Y, include_header=include_header, overwrite=overwrite)

    # ---- training -----------------------------------------------------------------------------
    def train_gp(self):
        """RBF(0.5) + WhiteKernel(0.1), alpha=1e-4, normalize_y, one optimiser restart
        (simple_gp.py:156-185); failures leave the model untrained instead of raising."""
        if len(self.X_train) < 30:
            return
        self._paths = None
        try:
            X = np.array(list(self.X_train))
            Y = np.array(list(self.Y_train))
            kernel = RBF(length_scale=0.5) + WhiteKernel(noise_level=0.1)
            self.gp_model = GaussianProcessRegressor(kernel=kernel, alpha=1e-4, normalize_y=True,
                                                     n_restarts_optimizer=1, device=self.device,
                                                     predict_dtype=self.predict_dtype)
            self.gp_model.fit(X, Y)
            self.is_trained = True
            self.training_count += 1
            print(f"Simple GP trained with {len(X)} samples (iteration {self.training_count})")
        except Exception as e:  # noqa: BLE001 - reference behaviour: report and stay untrained
            print(f"GP training failed: {e}")
            self.is_trained = False

    def load_model(self, model_path):
        """Reads the `{'gp_model', 'training_count', ...}` pickle of train_gp_offline.py:188-194.
        A scikit-learn regressor inside it is ingested onto the GPU as is."""
        self._paths = None
        try:
            if not os.path.exists(model_path):
                print(f"Model file not found: {model_path}")
                return False
            with open(model_path, "rb") as f:
                model_data = pickle.load(f)
            model = model_data["gp_model"]
            if not isinstance(model, GaussianProcessRegressor) and hasattr(model, "L_") and hasattr(model, "kernel_"):
                model = GaussianProcessRegressor.from_sklearn(model, device=self.device,
                                                              predict_dtype=self.predict_dtype)
            self.gp_model = model
            self.is_trained = True
            self.training_count = model_data.get("training_count", 0)
            print(f"GP model loaded: {model_path} (samples: {model_data.get('data_points_used', 'unknown')}, "
                  f"created: {model_data.get('timestamp', 'unknown')})")
            return True
        except Exception as e:  # noqa: BLE001
            print(f"Failed to load model: {e}")
            return False

    # ---- prediction ---------------------------------------------------------------------------
    def predict_residual(self, state, control):
        """One row -> (mean (6,), variance = std^2 (6,)); untrained/failed -> (zeros, ones)
        (simple_gp.py:187-201)."""
        if not self.is_trained:
            return np.zeros(6), np.ones(6)
        try:
            x = np.concatenate([state, control]).reshape(1, -1)
            mean, std = self.gp_model.predict(x, return_std=True)
            self.prediction_count += 1
            return mean.flatten(), std.flatten() ** 2
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros(6), np.ones(6)

    def predict_residual_jacobian(self, state, control):
        """One row -> (mean (6,), J (6, 10)): the residual and its Jacobian with respect to [state(6), control(4)], one
        launch (`GaussianProcessRegressor.predict_jacobian`); untrained/failed -> (zeros(6), zeros((6, 10))), never raising
        into the control loop."""
        if not self.is_trained:
            return np.zeros(6), np.zeros((6, 10))
        try:
            x = np.concatenate([state, control]).reshape(1, -1)
            mean, J = self.gp_model.predict_jacobian(x)
            self.prediction_count += 1
            return mean.reshape(-1), J.reshape(mean.size, -1)
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros(6), np.zeros((6, 10))

    def predict_residual_hessian(self, state, control):
        """One row -> (mean (6,), J (6, 10), H (6, 10, 10)): the residual with its first and second derivatives with respect
        to [state(6), control(4)], one call (`predict_hessian` of the exact or the sparse model); untrained/failed -> zeros of
        these shapes and a printed reason, never raising into the control loop."""
        zeros = np.zeros(6), np.zeros((6, 10)), np.zeros((6, 10, 10))
        if not self.is_trained:
            print("GP Hessian unavailable: the model is not trained")
            return zeros
        try:
            x = np.concatenate([state, control]).reshape(1, -1)
            mean, J, H = self.gp_model.predict_hessian(x)
            self.prediction_count += 1
            D = x.shape[1]
            return mean.reshape(-1), J.reshape(mean.size, D), H.reshape(mean.size, D, D)
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return zeros

    def predict_residual_batch(self, X, return_var=True):
        """M rows [state(6), control(4)] in one kernel call -> (mean (M,P), variance (M,P))."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        P = 6 if self.gp_model is None else int(np.size(self.gp_model._y_train_std))      # (exact and sparse models both)
        if not self.is_trained:
            return np.zeros((len(X), P)), np.ones((len(X), P))
        try:
            if return_var:
                mean, std = self.gp_model.predict(X, return_std=True)
                self.prediction_count += len(X)
                return mean.reshape(len(X), -1), std.reshape(len(X), -1) ** 2
            mean = self.gp_model.predict(X)
            self.prediction_count += len(X)
            return mean.reshape(len(X), -1), None
        except Exception as e:  # noqa: BLE001
            print(f"GP prediction failed: {e}")
            return np.zeros((len(X), P)), np.ones((len(X), P))

    def build_gp_residuals(self, X_guess, U_guess, dt, gain=0.1, n_states=6):
        """Horizon-batched counterpart of `QuadrotorMPC._build_gp_residuals`
        (src/px4/mpc.py:1475-1511): D[3:6, k] = gain * mean_k[3:6] / dt for every stage k, from
        ONE batched mean prediction.  X_guess (6, N+1) or (R, 6, N+1) for R rollouts;
        U_guess (4, N) / (R, 4, N).  Returns D (6, N) / (R, 6, N)."""
        X_guess = np.asarray(X_guess, dtype=float)
        U_guess = np.asarray(U_guess, dtype=float)
        single = X_guess.ndim == 2
        if single:
            X_guess, U_guess = X_guess[None], U_guess[None]
        R, _, N = U_guess.shape
        D = np.zeros((R, n_states, N))
        if self.is_trained:
            rows = np.concatenate([X_guess[:, :6, :N], U_guess[:, :4, :]], axis=1)    # (R, 10, N)
            rows = rows.transpose(0, 2, 1).reshape(R * N, -1)
            mean, _ = self.predict_residual_batch(rows, return_var=False)
            if mean.shape[1] >= n_states:
                acc = gain * (mean / dt)[:, 3:6].reshape(R, N, 3)
                D[:, 3:6, :] = acc.transpose(0, 2, 1)
        return D[0] if single else D

    def linearize_gp_residuals(self, X_guess, U_guess, dt, gain=0.1, n_states=6):
        """First-order companion of `build_gp_residuals`: the frozen residual D and its linearisation around the guess,
        for an MPC that builds A, B per stage (quadrotor_gp_mpc/quadrotor_gp_mpc/mpc_controller.py:318).  Returns
        (D, A, B): D (6, N) as `build_gp_residuals` returns it; A (N, 6, 6) and B (N, 6, 4), zero except rows 3:6 =
        gain / dt * J_k[3:6, :6] and gain / dt * J_k[3:6, 6:10], J_k the Jacobian of the residual mean at stage k - from
        ONE call for the whole horizon.  (R, ...) leading axis for R rollouts as in `build_gp_residuals`; untrained or a
        failed prediction: zeros."""
        X_guess = np.asarray(X_guess, dtype=float)
        U_guess = np.asarray(U_guess, dtype=float)
        single = X_guess.ndim == 2
        if single:
            X_guess, U_guess = X_guess[None], U_guess[None]
        R, _, N = U_guess.shape
        D = np.zeros((R, n_states, N))
        A = np.zeros((R, N, n_states, 6))
        B = np.zeros((R, N, n_states, 4))
        if self.is_trained:
            rows = np.concatenate([X_guess[:, :6, :N], U_guess[:, :4, :]], axis=1)    # (R, 10, N)
            rows = rows.transpose(0, 2, 1).reshape(R * N, -1)
            try:
                mean, J = self.gp_model.predict_jacobian(rows)
                self.prediction_count += len(rows)
                mean = mean.reshape(R * N, -1)
                J = J.reshape(R * N, mean.shape[1], -1)
                if mean.shape[1] >= n_states:
                    D[:, 3:6, :] = (gain * (mean / dt)[:, 3:6]).reshape(R, N, 3).transpose(0, 2, 1)
                    A[:, :, 3:6, :] = (gain / dt * J[:, 3:6, :6]).reshape(R, N, 3, 6)
                    B[:, :, 3:6, :] = (gain / dt * J[:, 3:6, 6:10]).reshape(R, N, 3, 4)
            except Exception as e:  # noqa: BLE001
                print(f"GP prediction failed: {e}")
                D[:], A[:], B[:] = 0.0, 0.0, 0.0
        if single:
            return D[0], A[0], B[0]
        return D, A, B

    def predict_horizon_gated(self, X_guess, U_guess, confidence_threshold, n_states=6):
        """Batched counterpart of `_get_gp_predictions_for_horizon`
        (src/px4/mpc_direct_rates.py:317-355): one mean+variance call for the whole horizon; stage k keeps
        the GP residual only if sqrt(sum_p var_kp) < confidence_threshold, otherwise zeros (nominal
        dynamics).  Returns (N, n_states)."""
        X_guess = np.asarray(X_guess, dtype=float)
        U_guess = np.asarray(U_guess, dtype=float)
        N = U_guess.shape[1]
        out = np.zeros((N, n_states))
        if not self.is_trained:
            return out
        rows = np.concatenate([X_guess[:6, :N], U_guess[:4, :N]], axis=0).T
        mean, var = self.predict_residual_batch(rows, return_var=True)
        keep = np.sqrt(np.sum(var, axis=1)) < confidence_threshold
        out[keep] = mean[keep, :n_states]
        return out

    def sample_rollouts(self, state, U_guess, dt, n_rollouts=64, n_features=1024, random_state=0, return_jacobian=False):
        """`n_rollouts` closed-loop rollouts under the model's own uncertainty: rollout r follows ONE posterior function draw
        along the whole horizon, stage k + 1 evaluated at the state its sampled residual of stage k produced,

            x_{k+1} = x_k + dt [v_k, a_k] + f_r([x_k, u_k])

        in one call for the horizon (`PosteriorPaths.rollout`).  state (6,); U_guess (4, N).  Returns (R, 6, N + 1), the layout
        `build_gp_residuals` / `linearize_gp_residuals` take as X_guess.  The path set (n_rollouts, n_features, random_state)
        is drawn once and cached on the object until `train_gp` / `load_model` - or, for a `SparseGP` as `gp_model`
        (`SparseGP.sample_paths`), until that model takes rows or is retrained: the same functions from call to call.
        Untrained, or on any failure (printed): the nominal trajectory repeated R times - it never raises into the control
        loop.

        return_jacobian=True: (X, J) in one call (`PosteriorPaths.rollout(..., return_jacobian=True)`); X as above, with the
        same bits; J (R, N, 6, 10): J[r, k] is the Jacobian of the SAMPLED residual f_r at [x_k, u_k] of rollout r - the
        function that produced the rollout, not the posterior mean `linearize_gp_residuals` linearises.  With the `lin` of the
        nominal double integrator (`paths.nominal_rollouts`) the stage matrices of rollout r's closed loop are
        A_k = I + lin[:, :6] + J[r, k][:, :6] and B_k = lin[:, 6:] + J[r, k][:, 6:] (no gain / dt factor: J already is the
        derivative of the state increment).  Untrained or failed: the nominal trajectory and a zero J."""
        from .paths import cached_path_set, nominal_rollouts, roll_paths
        state = np.asarray(state, dtype=float).reshape(-1)[:6]
        U_guess = np.asarray(U_guess, dtype=float)
        fallback, lin = nominal_rollouts(self._nominal_dynamics, state, U_guess, dt, n_rollouts)
        if return_jacobian:
            fallback = (fallback, np.zeros((fallback.shape[0], U_guess.shape[1], 6, 10)))
        if not self.is_trained:
            return fallback
        try:
            paths = cached_path_set(self, "_paths", self.gp_model, n_rollouts, n_features, random_state)
            traj = roll_paths(paths, state, U_guess, lin, return_jacobian=True) if return_jacobian else \
                roll_paths(paths, state, U_guess, lin)
            self.prediction_count += int(n_rollouts) * U_guess.shape[1]
            return traj
        except Exception as e:  # noqa: BLE001
            print(f"GP rollout sampling failed: {e}")
            return fallback

    def propagate_horizon(self, state, U_guess, dt, Sigma0=None, process_noise=None, order=1, method="linear"):
        """The closed loop of the posterior MEAN with the state covariance the model's uncertainty induces along it, to first
        order, in one call for the horizon (`GaussianProcessRegressor.propagate`):

            x_{k+1} = x_k + dt [v_k, a_k] + mu([x_k, u_k]),   Sigma_{k+1} = A_k Sigma_k A_k^T + diag(var([x_k, u_k])) + Q

        with A_k = I + lin[:, :6] + d mu / d x - the covariances that tighten a cautious MPC's constraints.  state (6,);
        U_guess (4, N) -> X (6, N + 1), Sigma (N + 1, 6, 6); U_guess (R, 4, N) -> (R, 6, N + 1), (R, N + 1, 6, 6).  Sigma0
        (6, 6) (default zero) and process_noise (6, 6), symmetric.  The variances are the latent function's.  Untrained, or on
        any failure (printed): the nominal trajectory and the nominal propagation Sigma_{k+1} = (I + lin_x) Sigma_k (I +
        lin_x)^T + Q - it never raises into the control loop.  order=2: x_{k+1} also takes tr(H_b Sigma_k) / 2 per output b, H_b
        the state block of the mean's Hessian (`GaussianProcessRegressor.propagate`); any other order: ValueError.
        method="moment": the exact moments of the posterior at the Gaussian query of every stage instead of their linearisation
        (`GaussianProcessRegressor.propagate(method="moment")`; a SparseGP model: `SparseGP.propagate_moments`, one call for the
        horizon); ValueError with order=2."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.check_method(method, order)
        state, U, lin, nominal, single = _pg.horizon_inputs(self._nominal_dynamics, state, U_guess, dt)
        R, N = U.shape[0], U.shape[1]
        if not self.is_trained:
            print("GP horizon propagation: the model is not trained - nominal trajectory and covariance")
            return _pg.horizon_layout(*_pg.nominal_horizon(nominal, lin, Sigma0, process_noise), single)
        try:
            # (a SparseGP model: its one-call chain where it applies, the host loop otherwise; with method="moment" its
            # `propagate_moments`)
            traj, Sigma = _pg.model_horizon(self.gp_model, state, U, lin, order=order, method=method, Sigma0=Sigma0,
                                            process_noise=process_noise)
            if not (np.isfinite(traj).all() and np.isfinite(Sigma).all()):
                raise FloatingPointError("non-finite trajectory or covariance")
            self.prediction_count += R * N
            return _pg.horizon_layout(traj, Sigma, single)
        except Exception as e:  # noqa: BLE001
            print(f"GP horizon propagation failed: {e}")
            return _pg.horizon_layout(*_pg.nominal_horizon(nominal, lin, Sigma0, process_noise), single)

    def horizon_gradient(self, state, U_guess, dt, grad_traj, grad_Sigma=None, method="linear"):
        """`propagate_horizon` (first order, Sigma0 = 0, no process noise) with the gradient of a horizon cost l(X, Sigma) with
        respect to the controls and the start state, in one call (`GaussianProcessRegressor.propagate_gradient`).  grad_traj
        (N + 1, 6) = dl/dx_k, grad_Sigma (N + 1, 6, 6) = dl/dSigma_k (default zero); U_guess (4, N) -> X (6, N + 1), Sigma
        (N + 1, 6, 6), dU (N, 4), dx0 (6,); U_guess (R, 4, N) with seeds (N + 1, R, ...) -> a leading R on every result.
        Untrained, or on any failure (printed): the nominal horizon and the sweep through the nominal dynamics (A = I + lin_x,
        no variance terms) - it never raises into the control loop.  method="moment": the horizon of `propagate_horizon(method=
        "moment")` and the gradient through its exact moments (`GaussianProcessRegressor.propagate_moments_gradient`; a SparseGP
        model: `SparseGP.propagate_moments_gradient`, one call for the horizon)."""
        from . import propagate as _pg
        state, U, lin, nominal, single = _pg.horizon_inputs(self._nominal_dynamics, state, U_guess, dt)
        R, N = U.shape[0], U.shape[1]
        if not self.is_trained:
            print("GP horizon gradient: the model is not trained - nominal trajectory and sweep")
            return _pg.nominal_gradient(nominal, lin, grad_traj, single)
        try:
            _pg.check_method(method)
            if method == "moment":
                traj, Sigma, dU, dx0, _ = _pg.model_moments_gradient(self.gp_model, state, U, lin, grad_traj, grad_Sigma)
            else:
                traj, Sigma, dU, dx0, _ = self.gp_model.propagate_gradient(state, U, lin, grad_traj, grad_Sigma,
                                                                           route=_pg.wrapper_route(self.gp_model))
            if not all(np.isfinite(a).all() for a in (traj, Sigma, dU, dx0)):
                raise FloatingPointError("non-finite trajectory, covariance or gradient")
            self.prediction_count += R * N
            return _pg.gradient_layout(traj, Sigma, dU, dx0, single)
        except Exception as e:  # noqa: BLE001
            print(f"GP horizon gradient failed: {e}")
            return _pg.nominal_gradient(nominal, lin, grad_traj, single)

    def get_uncertainty(self, state, control):
        _, variance = self.predict_residual(state, control)
        return np.mean(np.sqrt(variance))

    def predict_enhanced_dynamics(self, state, control, dt):
        residual_mean, _ = self.predict_residual(state, control)
        return self._nominal_dynamics(state, control, dt) + residual_mean

    def get_stats(self):
        return {
            "is_trained": self.is_trained,
            "data_points": len(self.X_train),
            "training_iterations": self.training_count,
            "predictions_made": self.prediction_count,
            "sklearn_available": False,      # key kept for the reference's log lines; sklearn is not used
            "backend": "mi355x-hip",
        }


class SimpleGPEnhancedMPC:
    """Confidence-gated dynamics wrapper (simple_gp.py:226-260)."""

    def __init__(self, gp_model, confidence_threshold=0.5):
        self.gp_model = gp_model
        self.confidence_threshold = confidence_threshold
        self.gp_usage = 0
        self.nominal_usage = 0

    def enhanced_dynamics_function(self, state, control, dt):
        if not self.gp_model.is_trained:
            self.nominal_usage += 1
            return self.gp_model._nominal_dynamics(state, control, dt)
        if self.gp_model.get_uncertainty(state, control) < self.confidence_threshold:
            self.gp_usage += 1
            return self.gp_model.predict_enhanced_dynamics(state, control, dt)
        self.nominal_usage += 1
        return self.gp_model._nominal_dynamics(state, control, dt)

    def get_usage_ratio(self):
        total = self.gp_usage + self.nominal_usage
        return 0.0 if total == 0 else self.gp_usage / total * 100
