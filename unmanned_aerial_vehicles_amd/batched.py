"""B independent single-output ARD GPs that share their training inputs (BASELINE config 5: the per-axis
ax/ay/az models of `src/px4/gp_trainer.py:139-179`, one `C(1,fixed)*RBF(ls in R^D)+WhiteKernel` GP per
output).

* training / hyper-parameter steps: the B factorisations are independent, so each model runs on its own
  libgpk handle and HIP stream from a worker thread (ctypes releases the GIL) — at the small and medium
  N of this use case a single model's launch chain cannot fill 256 CUs, the B chains overlap;
* prediction: ONE fused launch evaluates all B posterior means (`gpk_predict_mean_multi`): the feature
  differences of a (query, training point) pair are formed once and reused by every model.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import dev_ptr as _p, host_ptr as _hp
from .device import Backend, check_queries, get_backend
from .gpr import GaussianProcessRegressor, cholesky_draws
from .kernels import RBF, ConstantKernel, WhiteKernel


class BatchedARDGP:
    def __init__(self, length_scale=1.0, length_scale_bounds=(0.1, 10.0), noise_level=0.01,
                 noise_level_bounds=(1e-5, 1e1), alpha=1e-6, normalize_y=True, optimizer="fmin_l_bfgs_b",
                 n_restarts_optimizer=0, device=None, predict_dtype="float64", concurrent=True):
        self.length_scale, self.length_scale_bounds = length_scale, length_scale_bounds
        self.noise_level, self.noise_level_bounds = noise_level, noise_level_bounds
        self.alpha, self.normalize_y = alpha, normalize_y
        self.optimizer, self.n_restarts_optimizer = optimizer, n_restarts_optimizer
        self.device, self.predict_dtype, self.concurrent = device, predict_dtype, concurrent
        self.models = []
        self._workers = []
        self._fused = None
        self._fs = None
        self._serve = None

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_workers"], st["_fused"], st["_fs"] = [], None, None   # handles, streams, device tensors: rebuilt lazily
        st["_serve"] = None
        st["_shared_x"] = None
        return st

    # ------------------------------------------------------------------ workers
    def _backend(self, b):
        import torch
        main = get_backend(self.device)
        if not self.concurrent:
            return main, None
        while len(self._workers) <= b:
            self._workers.append((Backend(main.device_index), torch.cuda.Stream(device=main.device)))
        return self._workers[b]

    def _map(self, fn, n):
        """Run fn(b) for b in range(n); concurrently (one stream + handle per model) when enabled."""
        import torch
        if not self.concurrent or n == 1:
            return [fn(b) for b in range(n)]

        def run(b):
            be, stream = self._backend(b)
            with torch.cuda.stream(stream):
                out = fn(b)
                stream.synchronize()
            return out

        for b in range(n):
            self._backend(b)
        torch.cuda.current_stream().synchronize()
        with ThreadPoolExecutor(max_workers=n) as ex:
            return list(ex.map(run, range(n)))

    def _kernel(self, D):
        ls = np.broadcast_to(np.asarray(self.length_scale, dtype=np.float64), (D,)).copy()
        return (ConstantKernel(1.0, constant_value_bounds="fixed") * RBF(ls, self.length_scale_bounds)
                + WhiteKernel(self.noise_level, self.noise_level_bounds))

    # ------------------------------------------------------------------ fit / LML
    def fit(self, X, Y):
        """Fit B single-output ARD GPs on the shared inputs X (N, D); Y is (N, B).

        With the L-BFGS-B optimiser and B > 1 the hyper-parameters of all models are optimised together: the
        objective is the sum of the B log-marginal likelihoods (block-separable, so the joint optimum is the
        per-model optimum) and every evaluation is ONE fused launch chain for all models.  Restarts draw a new
        start for every model at once and each model keeps its best run."""
        import scipy.optimize
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64).reshape(len(X), -1)
        B, D = Y.shape[1], X.shape[1]
        if B > 8:
            raise ValueError("at most 8 models per batch")
        joint = self.optimizer == "fmin_l_bfgs_b" and B > 1

        def one(b):
            be = self._backend(b)[0]
            g = GaussianProcessRegressor(kernel=self._kernel(D), alpha=self.alpha, normalize_y=self.normalize_y,
                                         optimizer=None if joint else self.optimizer,
                                         n_restarts_optimizer=self.n_restarts_optimizer,
                                         device=be, predict_dtype=self.predict_dtype)
            return g.fit(X, Y[:, b])

        self.models = self._map(one, B)
        self._fused = None
        self._fs = None
        if joint:
            nth = self.models[0].kernel_.n_dims
            bounds = np.tile(self.models[0].kernel_.bounds, (B, 1))

            def obj(flat):
                lml, grad = self._lml_fused(flat.reshape(B, nth), True)
                lml = np.where(np.isfinite(lml), lml, -1e25)          # a not-PD model: large penalty, zero gradient
                return -float(np.sum(lml)), -grad.reshape(-1)

            rng = np.random.mtrand._rand
            best_theta = self.thetas.copy()
            best_lml = np.full(B, -np.inf)
            starts = [self.thetas.reshape(-1)]
            starts += [rng.uniform(bounds[:, 0], bounds[:, 1]) for _ in range(self.n_restarts_optimizer)]
            for x0 in starts:
                res = scipy.optimize.minimize(obj, x0, method="L-BFGS-B", jac=True, bounds=bounds)
                th = res.x.reshape(B, nth)
                lml = self._lml_fused(th, False)
                better = lml > best_lml
                best_theta[better], best_lml[better] = th[better], lml[better]
            self.release_fused_buffers()

            def finish(b):
                g = self.models[b]
                g.kernel_.theta = best_theta[b]
                g.log_marginal_likelihood_value_ = float(best_lml[b])
                g._refactor()
                g._alpha_host = g._L_host = None
                return g

            self.models = self._map(finish, B)
        return self

    def log_marginal_likelihood(self, thetas, eval_gradient=False, fused=True):
        """thetas: (B, D+1) log-parameters [log ls_0..log ls_{D-1}, log noise] per model.
        Returns lml (B,) and, with eval_gradient, grad (B, D+1) — the hyper-parameter step of config 5.
        fused=True: the B factorisations, inversions and alpha solves share ONE launch chain (every kernel gets
        a batch grid dimension, `gpk_batch_begin`); fused=False: one chain per model on its own stream."""
        thetas = np.asarray(thetas, dtype=np.float64)
        if fused:
            return self._lml_fused(thetas, eval_gradient)

        def one(b):
            return self.models[b].log_marginal_likelihood(thetas[b], eval_gradient)

        res = self._map(one, len(self.models))
        if not eval_gradient:
            return np.array(res)
        return np.array([r[0] for r in res]), np.stack([r[1] for r in res])

    def _fused_state(self):
        """Stacked HBM buffers for the batched launch chain: K/L, leaf inverses, W = L^-1, K^-1, scratch."""
        import torch
        if getattr(self, "_fs", None) is None:
            m0 = self.models[0]
            for m in self.models:
                m._ensure_device()
            be = get_backend(self.device)
            B, N, D = len(self.models), m0._dev.N, m0._dev.D
            Np = m0._dev.Np
            tsz = (Np // 2 + 128) ** 2
            f64 = torch.float64
            # per-model rows of Yn / alpha are registered as batch buffers: gpk_batch_buffer wants strides that are
            # multiples of 16 bytes, so the rows are N rounded up to even long (an odd N - e.g. 241 of 302 samples
            # after the 80/20 split - otherwise fails with GPK_BAD_ARG)
            Ne = N + (N & 1)
            Yn = torch.zeros((B, Ne), dtype=f64, device=be.device)
            for b, m in enumerate(self.models):
                Yn[b, :N].copy_(m._dev.Yn[:, 0])
            self._fs = {
                "be": be, "B": B, "N": N, "Ne": Ne, "D": D, "Np": Np, "tsz": tsz,
                "X": m0._dev.X.to(be.device),
                "Yn": Yn,                                                                              # (B, Ne)
                "K": be.empty((B, Np, Np), f64), "winv": be.empty((B, Np, 128), f64),
                "W": be.empty((B, Np, Np), f64), "Kinv": be.empty((B, Np, Np), f64),
                "T": be.empty((B, tsz), f64), "alpha": be.empty((B, Ne), f64),
            }
        return self._fs

    def _lml_fused(self, thetas, eval_gradient):
        fs = self._fused_state()
        be, B, N, D, Np = fs["be"], fs["B"], fs["N"], fs["D"], fs["Np"]
        comps = [self.models[b].kernel_.clone_with_theta(thetas[b]).components() for b in range(B)]
        ls = [np.ascontiguousarray(c.ls_vector(D)) for c in comps]
        info = (C.c_int * B)()
        with be.lock:            # (the batched chain and the per-model terms read the stacked buffers: one sequence)
            for b in range(B):       # K1 per model (one launch each)
                be.call("gpk_gram", _lib.GPK_F64, _p(fs["X"]), N, D, _hp(ls[b]), comps[b].sf2,
                        (comps[b].noise or 0.0) + float(self.alpha), _p(fs["K"][b]), Np)
            be.call("gpk_batch_begin", B)
            try:
                for name, row_bytes in (("K", Np * Np * 8), ("winv", Np * 128 * 8), ("W", Np * Np * 8),
                                        ("Kinv", Np * Np * 8), ("T", fs["tsz"] * 8), ("Yn", fs["Ne"] * 8),
                                        ("alpha", fs["Ne"] * 8)):
                    be.call("gpk_batch_buffer", _p(fs[name]), row_bytes)
                rc = be.status("gpk_potrf", _p(fs["K"]), Np, Np, _p(fs["winv"]), info)          # K2, B problems
                if rc != _lib.GPK_NOT_PD:      # (a model that is not positive definite is a result: info[b] says which)
                    be.check(rc)
                be.call("gpk_trtri", _p(fs["K"]), Np, Np, _p(fs["winv"]), _p(fs["W"]), Np, _p(fs["T"]))
                be.call("gpk_potrs_inv", _p(fs["W"]), Np, Np, _p(fs["Yn"]), N, 1, _p(fs["alpha"]))   # K3
                if eval_gradient:
                    be.call("gpk_wtw", _p(fs["W"]), Np, Np, _p(fs["Kinv"]), Np)
            finally:
                be.status("gpk_batch_end")
            lml = np.full(B, -np.inf)
            grad = np.zeros((B, thetas.shape[1]))
            terms = np.zeros(2)
            g = np.zeros(D + 2)
            for b in range(B):
                if info[b] != 0:       # not positive definite: (-inf, 0) as sklearn/_gpr.py:588-589
                    continue
                be.call("gpk_lml_terms", _p(fs["K"][b]), N, Np, _p(fs["Yn"][b]), _p(fs["alpha"][b]), 1, _hp(terms))
                lml[b] = -0.5 * terms[1] - terms[0] - 0.5 * N * np.log(2.0 * np.pi)
                if eval_gradient:
                    be.call("gpk_lml_grad", _p(fs["X"]), N, D, _hp(ls[b]), comps[b].sf2, comps[b].noise or 0.0,
                            _p(fs["alpha"][b]), 1, _p(fs["Kinv"][b]), Np, _hp(g))
                    grad[b] = comps[b].map_gradient(g, D)
        return (lml, grad) if eval_gradient else lml

    def release_fused_buffers(self):
        self._fs = None

    @property
    def thetas(self):
        return np.stack([m.kernel_.theta for m in self.models])

    # ------------------------------------------------------------------ predict
    def _build_fused(self):
        import torch
        m0 = self.models[0]
        for m in self.models:
            m._ensure_device()
        be = get_backend(self.device)
        # fp32 serving is gated as in the estimator (DeviceGP, "fp32 serving gates"): if any model's fp32 mean would leave
        # the stated 1e-4, the whole fused call runs on the fp64 kernels
        f32 = self.predict_dtype == "float32" and all(m._dev.fp32_mean_ok() for m in self.models)
        tdt = torch.float32 if f32 else torch.float64
        comps = [m.kernel_.components() for m in self.models]
        D = m0.n_features_in_
        with torch.cuda.device(be.device):
            torch.cuda.synchronize()
            alpha = torch.stack([m._dev.alpha[:, 0].to(be.device) for m in self.models], dim=1).to(tdt).contiguous()
            X = m0._dev.X.to(be.device).to(tdt).contiguous()
        self._fused = {
            "X": X, "alpha": alpha, "N": X.shape[0], "D": D, "tdt": tdt, "code": _lib.GPK_F32 if f32 else _lib.GPK_F64,
            "ls": np.ascontiguousarray(np.stack([c.ls_vector(D) for c in comps])),
            "sf2": np.ascontiguousarray([c.sf2 for c in comps], dtype=np.float64),
            "ym": np.ascontiguousarray([m._y_train_mean[0] for m in self.models], dtype=np.float64),
            "ys": np.ascontiguousarray([m._y_train_std[0] for m in self.models], dtype=np.float64),
        }

    MFMA_MIN_QUERIES = 1024      # below this the single fused launch wins on latency

    def predict_mean_dev(self, Xq):
        """All B posterior means (one fused launch, or one matrix-core launch per model for large fp32
        batches); returns a (M, B) device tensor."""
        import torch
        if self._fused is None:
            self._build_fused()
        f = self._fused
        be = get_backend(self.device)
        if isinstance(Xq, torch.Tensor):
            q = Xq.to(device=be.device, dtype=f["tdt"]).contiguous()
        else:
            q = be.upload(np.ascontiguousarray(Xq, dtype=np.float64), f["tdt"])
        M = q.shape[0]
        if (f["code"] == _lib.GPK_F32 and M >= self.MFMA_MIN_QUERIES
                and all(m._dev.mean_kernel_choice() == "mfma" for m in self.models)):
            # large fp32 batches: one matrix-core launch per model (distances on the bf16 MFMA pipe) beats the
            # fused vector-ALU kernel (0.115 vs 0.158 ms at N = 4096, 10 000 queries, B = 3)
            cols = [m._dev.predict_mean_dev(q, m._y_train_mean, m._y_train_std, "float32", "mfma") for m in self.models]
            return torch.cat(cols, dim=1)
        return self._fused_mean(f, q)

    def _fused_mean(self, f, q):
        """`gpk_predict_mean_multi`: the posterior means of all B models at the rows q (a device tensor of f's dtype) in one
        launch on the buffers f (`_fused` or `_fused64()`); returns the (M, B) tensor."""
        be = get_backend(self.device)
        M, B = q.shape[0], len(self.models)
        out = be.empty((M, B), f["tdt"])
        if M > 0:
            be.call("gpk_predict_mean_multi", f["code"], _p(f["X"]), _p(f["alpha"]), f["N"], f["D"], B, _hp(f["ls"]),
                    _hp(f["sf2"]), _hp(f["ym"]), _hp(f["ys"]), _p(q), M, _p(out))
        return out

    # ------------------------------------------------------------------ control-loop batches
    SERVE_MAX_M = 32

    @staticmethod
    def _alike(devs):
        """The models can share a launch: all factored, one output each, the same N and D, on one device."""
        d0 = devs[0]
        return all(d.factored and d.P == 1 and d.N == d0.N and d.D == d0.D and d.be.device == d0.be.device for d in devs)

    def _serve_state(self, want_std, any_dtype=False):
        """Argument block of `gpk_predict_host_multi` (one call, two launches for all models), or None when the
        models do not qualify: fp64 serving, single-output models on one device with the same training-set size,
        D <= 16, N <= 16384, at most 8 of them.  Rebuilt when a model has been refitted.  any_dtype: the caller runs
        the fp64 kernels whatever `predict_dtype` says (the input gradients)."""
        import torch
        ms = self.models
        if (self.predict_dtype == "float32" and not any_dtype) or not (1 <= len(ms) <= 8):
            return None
        for m in ms:
            m._ensure_device()
        devs = [m._dev for m in ms]
        key = tuple((id(d), id(d.ls), d.factored) for d in devs)
        sv = getattr(self, "_serve", None)
        if sv is None or sv["key"] != key:
            d0 = devs[0]
            if not self._alike(devs) or d0.D > 16 or d0.Np > 16384:
                self._serve = {"key": key, "ok": False}
                return None
            comps = [m.kernel_.components() for m in ms]
            B = len(ms)
            vp = C.c_void_p * B
            sv = self._serve = {
                "key": key, "ok": True, "B": B, "dev0": d0, "keep": devs,
                "X": vp(*[d.X.data_ptr() for d in devs]), "alpha": vp(*[d.alpha.data_ptr() for d in devs]),
                "ls": np.ascontiguousarray(np.stack([d.ls for d in devs])),
                "sf2": np.ascontiguousarray([d.sf2 for d in devs], dtype=np.float64),
                "ym": np.ascontiguousarray([m._y_train_mean[0] for m in ms], dtype=np.float64),
                "ys": np.ascontiguousarray([m._y_train_std[0] for m in ms], dtype=np.float64),
                "kss": np.ascontiguousarray([c.sf2 + (c.noise or 0.0) for c in comps], dtype=np.float64),
                "W": None,
            }
            with torch.cuda.device(d0.be.device):
                torch.cuda.synchronize()          # the models may have been fitted on their own streams
        if not sv["ok"]:
            return None
        if want_std and sv["W"] is None:
            if not all(d.host_path_ok(1, True) for d in sv["keep"]):
                return None
            Ws = [d.inverse_factor(False) for d in sv["keep"]]
            with torch.cuda.device(sv["dev0"].be.device):
                torch.cuda.synchronize()
            sv["Wt"] = Ws
            sv["W"] = (C.c_void_p * sv["B"])(*[w.data_ptr() for w in Ws])
        return sv

    def predict_host(self, Xq, return_std=False):
        """<= 32 rows, all models, one C call: (mean (M, B), std (M, B) or None); None if the models do not qualify."""
        st = self._host_queries(Xq, want_W=return_std, any_dtype=False, row_gate=False)
        if st is None:
            return None
        sv, Xq, M = st
        B = sv["B"]
        mean = np.empty((B, M))
        var = np.empty((B, M)) if return_std else None
        self._host_call("gpk_predict_host_multi", sv, return_std, sv["kss"].ctypes.data, 0.0, _hp(Xq), M, _hp(mean), _hp(var))
        if not return_std:
            return mean.T, None
        return mean.T, (np.sqrt(var) * sv["ys"][:, None]).T

    # What the one-call entries over all models (gpk_predict_host_multi / _multi_grad / _multi_cov) share, in two steps so that
    # a caller can size its outputs in between.  They run at the control rate: no closure, no argument list built per call.
    def _host_queries(self, Xq, want_W, any_dtype, row_gate):
        """(the serve state of `_serve_state(want_W, any_dtype)`, the queries as a contiguous float64 (M, D) array, M) - or
        None when the models do not qualify or, with `row_gate`, M is outside 1 .. SERVE_MAX_M."""
        sv = self._serve_state(want_W, any_dtype)
        if sv is None:
            return None
        Xq = np.ascontiguousarray(Xq, dtype=np.float64)
        D = sv["dev0"].D
        if Xq.ndim != 2 or Xq.shape[1] != D:
            raise ValueError(f"queries must be (M, {D})")
        M = Xq.shape[0]
        if row_gate and not (1 <= M <= self.SERVE_MAX_M):
            return None
        return sv, Xq, M

    def _host_call(self, entry, sv, want_W, *tail):
        """`entry(handle, the models' argument block, W or NULL, Np, ldw, *tail)`: `tail` is what follows in the entry's own
        order - its scalars, the queries' address, M, the outputs' addresses."""
        d0 = sv["dev0"]
        head = sv.get("head")
        if head is None:        # (the leading arguments, addresses included, once per serve state: each conversion costs per call)
            head = sv["head"] = (sv["B"], sv["X"], sv["alpha"], d0.N, d0.D, sv["ls"].ctypes.data, sv["sf2"].ctypes.data,
                                 sv["ym"].ctypes.data, sv["ys"].ctypes.data)
        d0.be.call(entry, *head, sv["W"] if want_W else None, d0.Np, d0.Np, *tail)

    # ------------------------------------------------------------------ input gradients (K8, per-axis batch)
    def predict_host_grad(self, Xq, return_var=False):
        """<= 32 rows, all models, one C call (`gpk_predict_host_multi_grad`: mean + Jacobian of every model in ONE launch,
        with the variances and their gradients three): (mean (M, B), dmean (M, B, D), var (M, B) or None, dvar (M, B, D) or
        None), var / dvar in target units (times y_std^2), dvar the gradient of the unclipped variance.  None if the models
        do not qualify (the conditions of `_serve_state`).  Always the fp64 kernels: an fp32-serving batch is served too."""
        st = self._host_queries(Xq, want_W=return_var, any_dtype=True, row_gate=True)
        if st is None:
            return None
        sv, Xq, M = st
        B, D = sv["B"], sv["dev0"].D
        mean, dmean = np.empty((B, M)), np.empty((B, M, D))
        var, dvar = (np.empty((B, M)), np.empty((B, M, D))) if return_var else (None, None)
        self._host_call("gpk_predict_host_multi_grad", sv, return_var, sv["kss"].ctypes.data, 0.0, _hp(Xq), M,
                        _hp(mean), _hp(var), _hp(dmean), _hp(dvar))
        mean, dmean = mean.T, dmean.transpose(1, 0, 2)
        if not return_var:
            return mean, dmean, None, None
        s2 = sv["ys"] ** 2
        return mean, dmean, (var * s2[:, None]).T, (dvar * s2[:, None, None]).transpose(1, 0, 2)

    # ------------------------------------------------------------------ exact moment matching (K11, per-axis batch)
    def _moments_state(self):
        """The serve state of `_serve_state` with every model's K^-1 (`DeviceGP.inverse_gram`, formed once per fit) as the
        pointer array "Kinv"; ValueError where the models do not qualify for the one-call entries."""
        import torch
        sv = self._serve_state(True, any_dtype=True)
        if sv is None or not all(d.moments_ok() for d in sv["keep"]):
            raise ValueError("exact moment matching needs the batch's one-call path: at most 8 single-output models of equal "
                             "size on one device, at most 16384 training rows, D <= 16, small_path != 0")
        if sv.get("Kinv") is None:
            Ks = [d.inverse_gram() for d in sv["keep"]]
            with torch.cuda.device(sv["dev0"].be.device):
                torch.cuda.synchronize()          # (formed on the models' own streams)
            sv["Kt"] = Ks
            sv["Kinv"] = (C.c_void_p * sv["B"])(*[k.data_ptr() for k in Ks])
        return sv

    def _moments_call(self, entry, sv, ym, ys, kss, *tail):
        d0 = sv["dev0"]
        try:
            d0.be.call(entry, sv["B"], sv["X"], sv["alpha"], d0.N, d0.D, _hp(sv["ls"]), _hp(sv["sf2"]), _hp(ym), _hp(ys), sv["Kinv"],
                       d0.Np, d0.Np, _hp(kss), 0.0, 0, None, *tail)
        except _lib.GPKError as e:      # a limit of the entry: the caller's arguments, with the library's message
            if e.code == _lib.GPK_BAD_ARG:
                raise ValueError(str(e)) from None
            raise

    def predict_moments(self, X, Sigma, in_scaler=None, out_scaler=None, var_includes_noise=False):
        """`GaussianProcessRegressor.predict_moments` for the batch, in raw units: the joint posterior of the B models at GAUSSIAN
        queries q ~ N(X[m], Sigma[m]), all B (B + 1) / 2 pairs of models included.  X (M, D) raw, M <= 32; Sigma (M, nx, nx) or
        (nx, nx) the raw covariance of the leading nx coordinates, or None; in_scaler / out_scaler as `propagate`.  Returns
        (mean (M, B), cov (M, B, B), xcov (M, B, D) = Cov[q_d, y_b] per unit of the raw query and the raw output).  One C call
        (`gpk_moments_host_multi`, five launches for all models and pairs); ValueError where the models do not qualify for it."""
        from . import propagate as _pg
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B, D = len(self.models), self.models[0].n_features_in_
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, D)
        in_shift, in_scale, o_mean, o_scale = _pg.check_scalers(B, D, in_scaler, out_scaler)
        sv = self._moments_state()
        ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
        mean, cov, xcov = np.empty((M, B)), np.empty((M, B, B)), np.empty((M, B, D))
        self._moments_call("gpk_moments_host_multi", sv, ym, ys, sv["kss"] if var_includes_noise else sv["sf2"], nx, _hp(in_shift),
                           _hp(in_scale), _hp(X), _hp(S), M, _hp(mean), _hp(cov), _hp(xcov))
        return mean, cov, xcov

    def predict_moments_vjp(self, X, Sigma, grad_mean=None, grad_cov=None, grad_xcov=None, in_scaler=None, out_scaler=None,
                            var_includes_noise=False):
        """`GaussianProcessRegressor.predict_moments_vjp` for the batch, in raw units: `predict_moments` and, for the seeds
        grad_mean (M, B), grad_cov (M, B, B), grad_xcov (M, B, D) (None: zero), dX (M, D) and dSigma (M, nx, nx) per unit of the
        raw query and its raw covariance.  Returns (mean, cov, xcov, dX, dSigma), the first three with the bits of
        `predict_moments`.  One C call (`gpk_moments_vjp_host_multi`: ten launches for all models and pairs)."""
        from . import propagate as _pg
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B, D = len(self.models), self.models[0].n_features_in_
        X, S, M, nx = _pg.check_gaussian_queries(X, Sigma, D)
        gm, gc, gxc = _pg.check_moment_seeds(grad_mean, grad_cov, grad_xcov, M, B, D)
        in_shift, in_scale, o_mean, o_scale = _pg.check_scalers(B, D, in_scaler, out_scaler)
        sv = self._moments_state()
        ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
        mean, cov, xcov = np.empty((M, B)), np.empty((M, B, B)), np.empty((M, B, D))
        dX, dS = np.empty((M, D)), np.empty((M, nx, nx))
        self._moments_call("gpk_moments_vjp_host_multi", sv, ym, ys, sv["kss"] if var_includes_noise else sv["sf2"], nx, _hp(in_shift),
                           _hp(in_scale), _hp(X), _hp(S), M, _hp(mean), _hp(cov), _hp(xcov), _hp(gm), _hp(gc), _hp(gxc), _hp(dX),
                           _hp(dS))
        return mean, cov, xcov, dX, dS

    def propagate_moments_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, coord=None, in_scaler=None, Sigma0=None,
                                   process_noise=None, var_includes_noise=False, out_scaler=None, route="auto"):
        """`propagate(method="moment")` with the gradient of a horizon cost, in raw units:
        `GaussianProcessRegressor.propagate_moments_gradient` with the batch's conventions (coord, in_scaler, out_scaler as
        `propagate`).  Returns (traj, Sigma, dU (R, H, nu), dx0 (R, nx), dSigma0 (R, nx, nx)), traj and Sigma with the bits of
        `propagate(method="moment")`.  One C call per horizon for all models and pairs (`gpk_propagate_mm_grad_host_multi`);
        route="host": the sweep on the host over `predict_moments` and `predict_moments_vjp`."""
        from . import propagate as _pg
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B = len(self.models)
        D = self.models[0].n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route)
        nx = lin.shape[0]
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, nx)
        _pg.check_method("moment", 1, "propagate_moments_gradient", Sigma0=S0, process_noise=Q)
        if route == "host":
            kw = dict(in_scaler=in_scaler, out_scaler=out_scaler, var_includes_noise=var_includes_noise)
            return _pg.host_adjoint_moments(lambda q, S: self.predict_moments(q, S, **kw),
                                            lambda q, S, gm, gc, gxc: self.predict_moments_vjp(q, S, gm, gc, gxc, **kw),
                                            coord, x0, U, lin, S0, Q, R, H, gx, gS)
        sv = self._moments_state()
        ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
        traj, Sigma, more = _pg.horizon_call(
            lambda *t: self._moments_call("gpk_propagate_mm_grad_host_multi", sv, ym, ys, sv["kss"] if var_includes_noise else sv["sf2"],
                                          nx, (C.c_int * B)(*coord), _hp(in_shift), _hp(in_scale), *t),
            x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
        return (traj, Sigma, *more)

    # ------------------------------------------------------------------ horizon propagation (K11, per-axis batch)
    def propagate(self, x0, U, lin, coord=None, in_scaler=None, Sigma0=None, process_noise=None, var_includes_noise=False,
                  return_stages=False, out_scaler=None, route="auto", order=1, method="linear"):
        """The batch's own closed-loop horizon in raw units: mean trajectory and linearised state covariance
        (`propagate`'s module docstring has the recursion), with the conventions of `BatchedPosteriorPaths.rollout`: the state
        has nx = len(lin) coordinates, B <= nx <= D; model b drives state coordinate coord[b] (default 0 .. B - 1); the models
        read z = (q - in_shift) / in_scale (in_scaler: None, a pair (shift, scale) or an object with `mean_` / `scale_`);
        out_scaler (mean (B,), scale (B,)): an affine map mean[b] + scale[b] y behind every model's output (a trainer's target
        scaler).  x0 (nx,) or (R, nx), U (H, nu) or (R, H, nu), Sigma0 / process_noise as
        `GaussianProcessRegressor.propagate`.  Returns (traj (H + 1, R, nx), Sigma (H + 1, R, nx, nx)) and, with
        return_stages=True, {"mean" (H, R, B), "var" (H, R, B), "jac" (H, R, B, D)}: jac per unit of the RAW query.  One C call
        per horizon (`gpk_propagate_host_multi`, three launches per stage for all models) where `_serve_state` holds; otherwise
        (or with the backend option small_path=0, or route="host") the same recursion as a host loop over
        `predict_jacobian`.  order=2: the second-order mean of `GaussianProcessRegressor.propagate` (`gpk_propagate2_host_multi`,
        four launches per stage; the host loop contracts `predict_hessian`); the stages gain "corr" (H, R, B).
        method="moment": every stage's exact moments at the Gaussian query N([x_h, u_h], Sigma_h) (`predict_moments`: the models'
        cross-covariances through the shared query included) instead of their linearisation - one C call
        (`gpk_propagate_mm_host_multi`, five launches per stage), route="host" the same recursion as a host loop over
        `predict_moments`; the stages are {"mean" (H, R, B), "cov" (H, R, B, B), "xcov" (H, R, B, D)}; order=2 with it is a
        ValueError.  The default method="linear" is the first-order chain above, untouched."""
        from . import propagate as _pg
        order = _pg.check_order(order)
        _pg.check_method(method, order)
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B = len(self.models)
        D = self.models[0].n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route)
        nx = lin.shape[0]
        if method == "moment":
            _pg.check_method(method, order, Sigma0=S0, process_noise=Q)
            if route == "host":
                traj, Sigma, stages = _pg.host_loop_moments(
                    lambda q, S: self.predict_moments(q, S, in_scaler=in_scaler, out_scaler=out_scaler,
                                                      var_includes_noise=var_includes_noise), coord, x0, U, lin, S0, Q, R, H)
                return (traj, Sigma, stages) if return_stages else (traj, Sigma)
            sv = self._moments_state()
            ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
            traj, Sigma, more = _pg.horizon_call(
                lambda *t: self._moments_call("gpk_propagate_mm_host_multi", sv, ym, ys, sv["kss"] if var_includes_noise else sv["sf2"],
                                              nx, (C.c_int * B)(*coord), _hp(in_shift), _hp(in_scale), *t),
                x0, U, lin, S0, Q, R, H, ((B,), (B, B), (B, D)) if return_stages else None)
            return (traj, Sigma, dict(zip(("mean", "cov", "xcov"), more))) if return_stages else (traj, Sigma)
        sv = self._serve_state(True, any_dtype=True) if route == "auto" else None
        if sv is not None and int(sv["dev0"].be.options.get("small_path", 1)) != 0:
            d0 = sv["dev0"]
            ym, ys = sv["ym"], sv["ys"]
            if out_scaler is not None:
                ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
            # (the noise enters through the prior variance the clip starts from, as in predict_host_grad: the same bits)
            kss = sv["kss"] if var_includes_noise else sv["sf2"]
            traj, Sigma, more = _pg.horizon_call(
                lambda *t: d0.be.call("gpk_propagate_host_multi" if order == 1 else "gpk_propagate2_host_multi",
                                      *self._chain_models(sv, ym, ys, kss, nx, coord, in_shift, in_scale), *t),
                x0, U, lin, S0, Q, R, H, ((B,), (B,), (B, D)) if return_stages else None, None if order == 1 else order)
            return (traj, Sigma, dict(zip(("mean", "var", "jac", "corr"), more))) if return_stages else (traj, Sigma)
        stage = _pg.batch_stage(self.predict_jacobian, _pg.noise_levels(self.models), in_shift, in_scale, o_mean, o_scale,
                                var_includes_noise)
        hess_stage = _pg.batch_hess_stage(self.predict_hessian, in_shift, in_scale, o_scale) if order == 2 else None
        traj, Sigma, stages = _pg.host_loop(stage, coord, x0, U, lin, S0, Q, R, H, hess_stage)
        return (traj, Sigma, stages) if return_stages else (traj, Sigma)

    @staticmethod
    def _chain_models(sv, ym, ys, kss, nx, coord, in_shift, in_scale):
        """The arguments of the batch's chain entries ahead of the horizon's (`propagate.horizon_call` supplies those)."""
        d0, B = sv["dev0"], sv["B"]
        return (B, sv["X"], sv["alpha"], d0.N, d0.D, _hp(sv["ls"]), _hp(sv["sf2"]), _hp(ym), _hp(ys), sv["W"], d0.Np, d0.Np, _hp(kss),
                0.0, 0, None, nx, (C.c_int * B)(*coord), _hp(in_shift), _hp(in_scale))

    def propagate_gradient(self, x0, U, lin, grad_traj, grad_Sigma=None, coord=None, in_scaler=None, Sigma0=None,
                           process_noise=None, var_includes_noise=False, out_scaler=None, route="auto", order=1, method="linear"):
        """`propagate` with the gradient of a horizon cost, in raw units: `GaussianProcessRegressor.propagate_gradient` with the
        batch's conventions (coord, in_scaler, out_scaler as `propagate`).  grad_traj (H + 1, R, nx), grad_Sigma (H + 1, R, nx,
        nx); returns (traj, Sigma, dU (R, H, nu), dx0 (R, nx), dSigma0 (R, nx, nx)), traj and Sigma with the bits of
        `propagate`.  One C call per horizon for all models (`gpk_propagate_grad_host_multi`, six launches per stage) where
        `propagate` makes one; otherwise (or route="host") the sweep on the host over `predict_jacobian` and
        `predict_hessian`.  order: 1 only (ValueError)."""
        from . import propagate as _pg
        _pg.check_grad_order(order)
        _pg.refuse_moment(method, "propagate_gradient")
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        B = len(self.models)
        D = self.models[0].n_features_in_
        x0, U, lin, S0, Q, R, H, coord, in_shift, in_scale, o_mean, o_scale = _pg.check_batch(
            B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route)
        nx = lin.shape[0]
        gx, gS = _pg.check_seeds(grad_traj, grad_Sigma, R, H, nx)
        sv = self._serve_state(True, any_dtype=True) if route == "auto" else None
        if sv is not None and int(sv["dev0"].be.options.get("small_path", 1)) != 0:
            d0 = sv["dev0"]
            ym, ys = sv["ym"], sv["ys"]
            if out_scaler is not None:
                ym, ys = np.ascontiguousarray(o_mean + o_scale * sv["ym"]), np.ascontiguousarray(o_scale * sv["ys"])
            kss = sv["kss"] if var_includes_noise else sv["sf2"]
            traj, Sigma, more = _pg.horizon_call(
                lambda *t: d0.be.call("gpk_propagate_grad_host_multi",
                                      *self._chain_models(sv, ym, ys, kss, nx, coord, in_shift, in_scale), *t),
                x0, U, lin, S0, Q, R, H, seeds=(gx, gS))
            return (traj, Sigma, *more)
        stage = _pg.batch_stage(self.predict_jacobian, _pg.noise_levels(self.models), in_shift, in_scale, o_mean, o_scale,
                                var_includes_noise, with_dvar=True)
        hess_stage = _pg.batch_hess_stage(self.predict_hessian, in_shift, in_scale, o_scale)
        return _pg.host_adjoint(stage, hess_stage, coord, x0, U, lin, S0, Q, R, H, gx, gS)

    def _fused64(self):
        """The fp64 buffers of the fused launches (shared X, alpha as one column per model) - `_fused` itself unless the
        batch serves in fp32."""
        import torch
        if self._fused is None:
            self._build_fused()
        f = self._fused
        if f["code"] == _lib.GPK_F64:
            return f
        if f.get("f64") is None:
            be = get_backend(self.device)
            with torch.cuda.device(be.device):
                torch.cuda.synchronize()
                alpha = torch.stack([m._dev.alpha[:, 0].to(be.device) for m in self.models], dim=1).double().contiguous()
                X = self.models[0]._dev.X.to(be.device).double().contiguous()
            f["f64"] = dict(f, X=X, alpha=alpha, tdt=torch.float64, code=_lib.GPK_F64)
        return f["f64"]

    def predict_jacobian(self, Xq, return_var=False):
        """Posterior means of all B models and their Jacobians with respect to the inputs, and with return_var=True the
        variances and their input gradients: (mean (M, B), dmean (M, B, D)[, var (M, B), dvar (M, B, D)]).  var equals
        `predict(return_std=True)[1] ** 2`; dvar is the gradient of the unclipped variance (the gradient of the standard
        deviation is dvar / (2 std)).  Up to 32 rows: one C call (`predict_host_grad`); larger batches: the fused mean
        launch and the fused mean-Jacobian launch (`gpk_predict_mean_grad_multi`: the feature differences of a pair formed
        once for all models) plus one variance-gradient chain per model.  Always fp64, as
        `GaussianProcessRegressor.predict_jacobian`."""
        Xq = check_queries(Xq)
        if 1 <= Xq.shape[0] <= self.SERVE_MAX_M:
            out = self.predict_host_grad(Xq, return_var)
            if out is not None:
                return out if return_var else out[:2]
        return self._predict_jacobian_large(Xq, return_var)

    def _shared_inputs(self):
        """True when every model was fitted on the same training inputs - what the fused launches assume (they read model 0's
        X); checked once per set of fitted models."""
        key = tuple(id(m._dev) for m in self.models)
        c = getattr(self, "_shared_x", None)
        if c is None or c[0] != key:
            x0 = self.models[0].X_train_
            same = all(m.X_train_.shape == x0.shape and np.array_equal(m.X_train_, x0) for m in self.models[1:])
            c = self._shared_x = (key, same)
        return c[1]

    def _predict_jacobian_large(self, Xq, return_var=False):
        import torch
        for m in self.models:
            m._ensure_device()
        if not self._shared_inputs():
            # models on different inputs: nothing to fuse, one call per model (the one-call path takes each model's own X)
            outs = [m.predict_jacobian(Xq, return_var=return_var) for m in self.models]
            return tuple(np.stack([o[i] for o in outs], axis=1) for i in range(4 if return_var else 2))
        f = self._fused64()
        be = get_backend(self.device)
        q = be.upload(np.ascontiguousarray(Xq, dtype=np.float64), torch.float64)
        M, B, D = q.shape[0], len(self.models), f["D"]
        mean_d, dmean_d = self._fused_mean(f, q), be.empty((M, B, D), torch.float64)
        if M > 0:
            be.call("gpk_predict_mean_grad_multi", _p(f["X"]), _p(f["alpha"]), f["N"], D, B, _hp(f["ls"]), _hp(f["sf2"]),
                    _hp(f["ys"]), _p(q), M, _p(dmean_d))
        mean, dmean = mean_d.cpu().numpy(), dmean_d.cpu().numpy()
        if not return_var:
            return mean, dmean
        var, dvar = np.empty((M, B)), np.empty((M, B, D))
        for b, m in enumerate(self.models):      # W and the length-scales differ per model: nothing to share
            comp = m.kernel_.components()
            v, g = m._dev.predict_var_grad_dev(Xq, comp.sf2 + (comp.noise or 0.0), 0.0)
            s2 = float(m._y_train_std[0]) ** 2
            var[:, b], dvar[:, b, :] = v.cpu().numpy() * s2, g.cpu().numpy() * s2
        return mean, dmean, var, dvar

    # ------------------------------------------------------------------ second derivatives of the means (K8, per-axis batch)
    def predict_host_hess(self, Xq):
        """<= 32 rows, all models, one C call (`gpk_predict_host_multi_hess`: mean + Jacobian of every model in the one launch
        of `predict_host_grad`, then the small-batch Hessian launch for all models: two launches, one synchronisation): (mean (M, B), dmean (M, B, D),
        hess (M, B, D, D)).  None if the models do not qualify (the conditions of `_serve_state`).  Always fp64."""
        st = self._host_queries(Xq, want_W=False, any_dtype=True, row_gate=True)
        if st is None:
            return None
        sv, Xq, M = st
        B, d0 = sv["B"], sv["dev0"]
        D = d0.D
        mean, dmean, hess = np.empty((B, M)), np.empty((B, M, D)), np.empty((B, M, D, D))
        d0.be.call("gpk_predict_host_multi_hess", B, sv["X"], sv["alpha"], d0.N, D, sv["ls"].ctypes.data, sv["sf2"].ctypes.data,
                   sv["ym"].ctypes.data, sv["ys"].ctypes.data, _hp(Xq), M, _hp(mean), _hp(dmean), _hp(hess))
        return mean.T, dmean.transpose(1, 0, 2), hess.transpose(1, 0, 2, 3)

    def predict_hessian(self, Xq):
        """Posterior means of all B models with their first and second input derivatives: (mean (M, B), dmean (M, B, D),
        hess (M, B, D, D)); mean and dmean are those of `predict_jacobian(Xq)` bit for bit, every D x D block of hess is
        symmetric bit for bit.  Up to 32 rows: one C call (`predict_host_hess`), in which column b has the bits of model b
        served alone through the same call; larger batches (whose chunking depends on B: column b agrees with model b alone to
        rounding, not bit for bit): the fused launches of `predict_jacobian` and the fused Hessian launch
        (`gpk_predict_mean_hess_multi`: the feature differences of a pair and their products formed once for all models).
        Always fp64, as `GaussianProcessRegressor.predict_hessian`."""
        Xq = check_queries(Xq)
        if 1 <= Xq.shape[0] <= self.SERVE_MAX_M:
            out = self.predict_host_hess(Xq)
            if out is not None:
                return out
        return self._predict_hessian_large(Xq)

    def _predict_hessian_large(self, Xq):
        mean, dmean = self._predict_jacobian_large(Xq)
        be = get_backend(self.device)
        import torch
        q = be.upload(np.ascontiguousarray(Xq, dtype=np.float64), torch.float64)
        if not self._shared_inputs():      # nothing to fuse: one call per model on its own inputs
            hess = np.stack([m._dev.predict_mean_hess_dev(q, m._y_train_std).cpu().numpy()[:, 0] for m in self.models], axis=1)
            return mean, dmean, hess
        f = self._fused64()
        M, B, D = q.shape[0], len(self.models), f["D"]
        hess_d = be.empty((M, B, D, D), torch.float64)
        if M > 0:
            be.call("gpk_predict_mean_hess_multi", _p(f["X"]), _p(f["alpha"]), f["N"], D, B, _hp(f["ls"]), _hp(f["sf2"]),
                    _hp(f["ys"]), _p(q), M, _p(hess_d))
        return mean, dmean, hess_d.cpu().numpy()

    # ------------------------------------------------------------------ joint posterior (K7, per-axis batch)
    def predict_host_cov(self, Xq):
        """<= 32 rows, all models, one C call (`gpk_predict_host_multi_cov`: two launches and one synchronisation for all of
        them): (mean (M, B), cov (M, M, B)), cov in target units (times y_std^2), each model's WhiteKernel level on its own
        diagonal, not clipped, symmetric bit for bit.  None if the models do not qualify (the conditions of `_serve_state`).
        Always the fp64 kernels: an fp32-serving batch is served too."""
        st = self._host_queries(Xq, want_W=True, any_dtype=True, row_gate=True)
        if st is None:
            return None
        sv, Xq, M = st
        if sv.get("noise") is None:
            sv["noise"] = np.ascontiguousarray([m.kernel_.components().noise or 0.0 for m in self.models], dtype=np.float64)
        mean, cov = np.empty((sv["B"], M)), np.empty((sv["B"], M, M))
        self._host_call("gpk_predict_host_multi_cov", sv, True, sv["noise"].ctypes.data, _hp(Xq), M, _hp(mean), _hp(cov))
        return mean.T, (cov * (sv["ys"] ** 2)[:, None, None]).transpose(1, 2, 0)

    def _predict_cov(self, Xq):
        """return_cov=True: up to 32 rows the one call; larger batches the fused mean launch plus each model's
        `predict_cov_dev`; models that do not qualify for either (different N, different devices, more than 8, different
        inputs): each model's own `predict(return_cov=True)`."""
        M, B = Xq.shape[0], len(self.models)
        if 1 <= M <= self.SERVE_MAX_M:
            out = self.predict_host_cov(Xq)
            if out is not None:
                return out
        for m in self.models:
            m._ensure_device()
        devs = [m._dev for m in self.models]
        fused = 1 <= B <= 8 and M >= 1 and self._alike(devs) and self._shared_inputs()
        if not fused:
            outs = [m.predict(Xq, return_cov=True) for m in self.models]
            return np.stack([o[0] for o in outs], axis=1), np.stack([o[1] for o in outs], axis=2)
        import torch
        f = self._fused64()
        be = get_backend(self.device)
        q = be.upload(np.ascontiguousarray(Xq, dtype=np.float64), torch.float64)
        mean = self._fused_mean(f, q).cpu().numpy()
        cov = np.empty((M, M, B))
        for b, m in enumerate(self.models):      # K*, W and the length-scales differ per model: nothing to share
            c = m._dev.predict_cov_dev(Xq, m.kernel_.components().noise or 0.0)
            cov[..., b] = c.contiguous().cpu().numpy() * float(m._y_train_std[0]) ** 2
        return mean, cov

    def sample_y(self, Xq, n_samples=1, random_state=0):
        """Draws from every model's joint posterior at the rows Xq: (M, B, n_samples).  Mean and covariance from
        `predict(Xq, return_cov=True)` (GPU); the draw on the host through the Cholesky factor of each covariance
        (`gpr.cholesky_draws`: one standard-normal block for all models, a stable function of the covariance)."""
        mean, cov = self.predict(Xq, return_cov=True)
        return cholesky_draws(mean, cov, n_samples, random_state)

    def sample_paths(self, n_paths, n_features=1024, random_state=0):
        """`n_paths` posterior function draws of EVERY model as explicit functions (`paths.BatchedPosteriorPaths`): evaluated
        anywhere, call after call, all models in one call - `step` two launches, a closed-loop `rollout` one call per horizon.
        The draw order is `paths.draw_batch_path_randomness`'s (model by model from the one generator); random_state as in
        `sample_y`.  Needs what the fused launches need - fitted single-output models of one size on one device and on the same
        training inputs - at most 8 of them, D <= 16, and no serving replica: a ValueError / RuntimeError names what is missing."""
        from .gpr import _rng_from
        from .paths import BatchedPosteriorPaths, check_batch_path_shape, draw_batch_path_randomness
        if not self.models:
            raise RuntimeError("this BatchedARDGP is not fitted yet")
        for m in self.models:
            m._ensure_device()
        d0 = self.models[0]._dev
        check_batch_path_shape(len(self.models), d0.D, int(n_paths), int(n_features))
        comps = [m.kernel_.components() for m in self.models]
        r = draw_batch_path_randomness(_rng_from(random_state), d0.N, d0.D, int(n_features), int(n_paths),
                                       np.stack([c.ls_vector(d0.D) for c in comps]),
                                       [(c.noise or 0.0) + float(m.alpha) for c, m in zip(comps, self.models)])
        return BatchedPosteriorPaths.from_randomness(self, **r)

    def predict(self, Xq, return_std=False, return_cov=False):
        """Means (M, B); with return_std the standard deviations (M, B); with return_cov=True every model's joint posterior
        covariance over the rows, (mean (M, B), cov (M, M, B)) in target units as scikit-learn scales it
        (`sklearn/gaussian_process/_gpr.py:441-469`, model by model).  The covariance always comes from the fp64 kernels."""
        if return_std and return_cov:
            raise RuntimeError("At most one of return_std or return_cov can be requested.")
        if return_cov:
            return self._predict_cov(check_queries(Xq))
        Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
        if 1 <= Xq.shape[0] <= self.SERVE_MAX_M:
            out = self.predict_host(Xq, return_std)
            if out is not None:
                return out if return_std else out[0]
        mean = self.predict_mean_dev(Xq).double().cpu().numpy()
        if not return_std:
            return mean
        std = np.stack(self._map(lambda b: self.models[b].predict(Xq, return_std=True)[1], len(self.models)), axis=1)
        return mean, std
