"""Horizon propagation: the posterior's mean rollout with the linearised state covariance (K11).

For a state x in R^nx, a query q = [x, u] in R^D and the nominal increment `lin` (nx x D, as `paths.nominal_rollouts` builds it):

    x_{h+1}     = x_h + lin q + sum_b e_coord[b] mu_b(q)
    A_h         = I + lin[:, :nx] + sum_b e_coord[b] J_b[:nx]               J_b = d mu_b / d q
    Sigma_{h+1} = A_h Sigma_h A_h^T + sum_b v_b(q) e_coord[b] e_coord[b]^T + Q

- the first-order propagation of Hewing, Kabzan and Zeilinger (Cautious MPC using GP regression).  The estimators run it as one
C call per horizon (`gpk_propagate_host[_multi]`, and `gpk_sparse_propagate[_multi]` for route="chain" of the sparse classes: three
launches per stage, one synchronisation); what is
here is what they share on the host: the argument checks (before any device call), the same recursion as a host loop over a
model's `predict_jacobian(..., return_var=True)` - the "auto" and "host" routes of the sparse models, the route of exact models
beyond the small-batch path and of option small_path=0 - and what the control-loop wrappers (`propagate_horizon`) share, their nominal fallback included.

`order=2` on every `propagate` adds the second-order term of E[mu(x)] for x ~ N(x_h, Sigma_h) to the mean,

    c_b = 1/2 sum_{d,e < nx} H_b[d][e] Sigma_h[d][e],      x_{h+1} = (x_h + lin q + sum_b e_coord[b] mu_b) + sum_b e_coord[b] c_b,

H_b = d2 mu_b / dq2; A_h and Sigma_{h+1} stay as above.  The one-call entries (`gpk_propagate2_host[_multi]`,
`gpk_sparse_propagate2[_multi]`: four launches per stage) contract H with Sigma without forming it; `host_loop` takes a
second-order stage callback built from the class's own `predict_hessian`.

`propagate_gradient` on every class returns, with the horizon itself, the gradient of a differentiable cost l(X, Sigma) with
respect to the controls, the start state and the start covariance (first order only: the derivative of c_b holds third
derivatives of the mean).  The caller supplies the seeds gx[h] = dl/dx_h and gS[h] = dl/dSigma_h (entries taken as independent;
(gS + gS^T) / 2 is used); from lam_H = gx_H, Lam_H = sym(gS_H), for h = H - 1 .. 0 and c_b = coord[b]:

    F_h   = [I 0] + lin + sum_b e_c J_b                     (nx x D, all D columns of the Jacobian)
    G_h   = Lam_{h+1} A_h Sigma_h,      w_b = [G_h[c_b, :nx], 0 .. 0]
    g_q   = F_h^T lam_{h+1} + sum_b Lam_{h+1}[c_b, c_b] grad_q v_b + 2 sum_b H_b w_b
    lam_h = gx_h + g_q[:nx],   dU_h = g_q[nx:],   Lam_h = sym(gS_h) + A_h^T Lam_{h+1} A_h

dx0 = lam_0, dSigma0 = Lam_0.  The one-call entries (`gpk_propagate_grad_host[_multi]`, `gpk_sparse_propagate_grad[_multi]`: six
launches per stage, one synchronisation) form H_b w_b without the Hessian; `host_adjoint` is the same sweep on the host over the
class's own `predict_jacobian(..., return_var=True)` and `predict_hessian`.

`method="moment"` on `propagate` of the exact classes replaces the linearisation of every stage by the exact moments of the
posterior at the Gaussian query N([x_h, u_h], Sigma_h) (`predict_moments`: mean, covariance V of the outputs and input-output
covariance; closed forms for RBF kernels):

    x_{h+1} = x_h + lin q + E mean,      Sigma_{h+1} = A0 Sigma_h A0^T + A0 Cx E^T + E Cx^T A0^T + E V E^T + Q

with A0 = I + lin[:, :nx], E the selector of `coord` and Cx the state rows of the input-output covariance (to first order Cx =
Sigma_h J_x^T, which gives the recursion at the top).  One C call per horizon (`gpk_propagate_mm_host[_multi]`: five launches per
stage, one synchronisation); `host_loop_moments` is the same recursion over a class's `predict_moments`.  The sparse classes
serve it as `predict_moments` / `propagate_moments` (the engine on (Z, alpha_u, Q = Kuu^-1 - Sigma~), `gpk_sparse_propagate_mm[_multi]`);
their `propagate(method="moment")` and every `propagate_gradient` refuse it (`refuse_moment`).

`propagate_moments_gradient` (every class; the sparse ones on (Z, alpha_u, Q): `gpk_sparse_propagate_mm_grad[_multi]`, which keeps
the stages' work blocks and runs five launches per stage forward and four backward) is the gradient of a horizon cost through that
recursion.  `predict_moments_vjp` returns, with the moments of a batch of Gaussian queries, the products of the seeds (on mean, cov and xcov) with their Jacobians
with respect to the query and its covariance (m~, S~; DESIGN.md section 4, K11, has the closed form).  With lam_{h+1}, Lam_{h+1} the
incoming adjoints the stage's seeds are E^T lam on the mean, E^T Lam E on cov and 2 E^T Lam A0 on the state columns of xcov, and

    g_q = [I 0]^T lam + lin^T lam + m~,   lam_h = gx_h + g_q[:nx],   dU_h = g_q[nx:],   Lam_h = sym(gS_h) + A0^T Lam A0 + S~

One C call per horizon (`gpk_propagate_mm_grad_host[_multi]`: six launches per stage forward, seven backward, one
synchronisation); `host_adjoint_moments` is the same sweep on the host over `predict_moments_vjp`.
"""
from __future__ import annotations

import numpy as np

from . import _lib

MAX_R, MAX_H, MAX_NX = 32, 256, 16


def horizon_call(call, x0, U, lin, S0, Q, R, H, stages=None, order=None, seeds=None):
    """The one C call of a horizon, for every class: `call(*tail)` makes it, with the entry's name and the model's arguments bound
    by the caller; x0 .. H as `check_horizon` returns them.  The tail every entry shares: x0 and its rows, U (null without
    controls) and its rows, lin, Sigma0 and its rows, Q, R, H, traj (H + 1, R, nx), Sigma (H + 1, R, nx, nx) and three stage
    arrays - (H, R) + each shape of `stages`, or null pointers with stages=None.  order (the second-order entries): then the
    order and corr, (H, R) + stages[0] or null.  seeds = (gx, gS) (the gradient entries): then the seeds and dU (R, H, nu), null
    without controls, dx0 (R, nx), dSigma0 (R, nx, nx).  Returns (traj, Sigma, more): the stage arrays (Nones with stages=None;
    corr last, given an order), or [dU, dx0, dSigma0].  ValueError, with the library's message, where the entry refuses its
    arguments."""
    hp = _lib.host_ptr
    nx, D = lin.shape
    traj, Sigma = np.empty((H + 1, R, nx)), np.empty((H + 1, R, nx, nx))
    more = [None] * 3 if stages is None else [np.empty((H, R) + tuple(s)) for s in stages]
    tail = [hp(a) for a in more]
    if order is not None:
        more.append(None if stages is None else np.empty((H, R) + tuple(stages[0])))
        tail += [int(order), hp(more[-1])]
    if seeds is not None:
        more = [np.zeros((R, H, D - nx)), np.empty((R, nx)), np.empty((R, nx, nx))]
        tail += [hp(seeds[0]), hp(seeds[1]), hp(more[0]) if D > nx else None, hp(more[1]), hp(more[2])]
    try:
        call(hp(x0), x0.shape[0], hp(U) if D > nx else None, U.shape[0], hp(lin), hp(S0), 1 if S0 is None else S0.shape[0], hp(Q), R, H,
             hp(traj), hp(Sigma), *tail)
    except _lib.GPKError as e:      # a limit of the entry: the caller's arguments, with the library's message
        if e.code == _lib.GPK_BAD_ARG:
            raise ValueError(str(e)) from None
        raise
    return traj, Sigma, more


def check_horizon(x0, U, lin, nx, D, Sigma0=None, process_noise=None):
    """The horizon's arguments as contiguous float64 arrays: (x0 (R or 1, nx), U (R or 1, H, nu), lin (nx, D), Sigma0 (R or 1, nx,
    nx) or None, Q (nx, nx) or None, R, H).  x0 is (nx,) or (R, nx), U (H, nu) or (R, H, nu), Sigma0 (nx, nx) or (R, nx, nx); R is
    inferred from them.  ValueError on a wrong shape, R > 32, H outside 1 .. 256, NaN or infinity, an asymmetric Sigma0 or
    process noise."""
    nx, D = int(nx), int(D)
    nu = D - nx
    if not (1 <= nx <= MAX_NX and nx <= D <= 16):
        raise ValueError(f"propagate: needs 1 <= nx <= D <= 16, got nx = {nx}, D = {D}")
    x0 = np.array(x0, dtype=np.float64, ndmin=2)
    if x0.ndim != 2 or x0.shape[1] != nx:
        raise ValueError(f"propagate: x0 must be ({nx},) or (R, {nx})")
    U = np.asarray(U, dtype=np.float64)
    if U.ndim == 2:
        U = U[None]
    if U.ndim != 3 or U.shape[2] != nu:
        raise ValueError(f"propagate: U must be (H, {nu}) or (R, H, {nu})")
    H = U.shape[1]
    if not (1 <= H <= MAX_H):
        raise ValueError(f"propagate: H must be in [1, {MAX_H}], got {H}")
    lin = np.asarray(lin, dtype=np.float64)
    if lin.shape != (nx, D):
        raise ValueError(f"propagate: lin must be ({nx}, {D})")
    S0 = None
    if Sigma0 is not None:
        S0 = np.asarray(Sigma0, dtype=np.float64)
        if S0.ndim == 2:
            S0 = S0[None]
        if S0.ndim != 3 or S0.shape[1:] != (nx, nx):
            raise ValueError(f"propagate: Sigma0 must be ({nx}, {nx}) or (R, {nx}, {nx})")
    Q = None
    if process_noise is not None:
        Q = np.asarray(process_noise, dtype=np.float64)
        if Q.shape != (nx, nx):
            raise ValueError(f"propagate: process_noise must be ({nx}, {nx})")
    rows = {a.shape[0] for a in (x0, U, S0) if a is not None and a.shape[0] != 1}
    if len(rows) > 1:
        raise ValueError(f"propagate: x0, U and Sigma0 disagree on the number of rollouts: {sorted(rows)}")
    R = rows.pop() if rows else 1
    if not (1 <= R <= MAX_R):
        raise ValueError(f"propagate: R must be in [1, {MAX_R}], got {R}")
    for name, a in (("x0", x0), ("U", U), ("lin", lin), ("Sigma0", S0), ("process_noise", Q)):
        if a is not None and not np.isfinite(a).all():
            raise ValueError(f"propagate: {name} contains NaN or infinity")
    if S0 is not None and not np.array_equal(S0, S0.transpose(0, 2, 1)):
        raise ValueError("propagate: Sigma0 must be symmetric")
    if Q is not None and not np.array_equal(Q, Q.T):
        raise ValueError("propagate: process_noise must be symmetric")
    c = np.ascontiguousarray
    return c(x0), c(U), c(lin), (None if S0 is None else c(S0)), (None if Q is None else c(Q)), R, H


def check_coord(coord, B, nx):
    """`coord` (default 0 .. B - 1) as a list of B distinct state coordinates in [0, nx)."""
    coord = list(range(B)) if coord is None else [int(c) for c in coord]
    if len(coord) != B or len(set(coord)) != B or not all(0 <= c < nx for c in coord):
        raise ValueError(f"propagate: coord must name {B} distinct state coordinates in [0, {nx})")
    return coord


def check_order(order):
    """`order` as 1 or 2; ValueError for anything else."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"propagate: order must be 1 or 2, got {order!r}")
    return int(order)


def host_loop(stage, coord, x0, U, lin, S0, Q, R, H, hess_stage=None):
    """The recursion on the host.  stage(q (R, D) raw) -> (mean (R, NO), jac (R, NO, D) per unit of the raw query, var (R, NO));
    output o drives state coordinate coord[o].  Returns traj (H + 1, R, nx), Sigma (H + 1, R, nx, nx) and the stage quantities
    {"mean" (H, R, NO), "var" (H, R, NO), "jac" (H, R, NO, D)}.
    hess_stage (second order): hess_stage(q (R, D) raw) -> the mean's Hessian (R, NO, D, D) per unit of the raw query; the
    stage's mean then takes c_o = tr(H_o[:nx, :nx] Sigma_h) / 2, added last, and the stages gain "corr" (H, R, NO)."""
    nx, D = lin.shape
    NO = len(coord)
    traj, Sigma = np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx))
    means, vars_, jacs = np.zeros((H, R, NO)), np.zeros((H, R, NO)), np.zeros((H, R, NO, D))
    corrs = np.zeros((H, R, NO))
    traj[0] = np.broadcast_to(x0, (R, nx))
    if S0 is not None:
        Sigma[0] = np.broadcast_to(S0, (R, nx, nx))
    eye_lin = np.eye(nx) + lin[:, :nx]
    for h in range(H):
        q = np.concatenate([traj[h], np.broadcast_to(U[:, h], (R, D - nx))], axis=1)
        mean, jac, var = stage(np.ascontiguousarray(q))
        means[h], vars_[h], jacs[h] = mean, var, jac
        x = traj[h] + q @ lin.T
        A = np.broadcast_to(eye_lin, (R, nx, nx)).copy()
        S = np.zeros((R, nx, nx))
        for o, c in enumerate(coord):
            x[:, c] += mean[:, o]
            A[:, c, :] += jac[:, o, :nx]
            S[:, c, c] = var[:, o]
        S += A @ Sigma[h] @ A.transpose(0, 2, 1)
        if Q is not None:
            S += Q
        if hess_stage is not None:
            hess = np.asarray(hess_stage(np.ascontiguousarray(q))).reshape(R, NO, D, D)
            corrs[h] = 0.5 * np.einsum("rode,rde->ro", hess[:, :, :nx, :nx], Sigma[h])
            for o, c in enumerate(coord):
                x[:, c] += corrs[h][:, o]
        traj[h + 1], Sigma[h + 1] = x, 0.5 * (S + S.transpose(0, 2, 1))
    stages = {"mean": means, "var": vars_, "jac": jacs}
    if hess_stage is not None:
        stages["corr"] = corrs
    return traj, Sigma, stages


# ---- exact moment matching (method="moment") ---------------------------------------------------------------------------------------
METHODS = ("linear", "moment")


def check_method(method, order=1, what="propagate", Sigma0=None, process_noise=None):
    """`method` as "linear" or "moment"; ValueError for anything else, and for "moment" with order=2 (the exact moments hold every
    order of the Taylor series: there is nothing to add to them) or with a Sigma0 or process noise (as `check_horizon` returns
    them) that is not positive semi-definite (`check_psd`)."""
    if method not in METHODS:
        raise ValueError(f"{what}: method must be 'linear' or 'moment', got {method!r}")
    if method == "moment" and order != 1:
        raise ValueError(f"{what}: method='moment' takes order=1 (the exact moments already hold the second-order term)")
    if method == "moment":
        check_psd(Sigma0, f"{what}: Sigma0")
        check_psd(process_noise, f"{what}: process_noise")
    return method


def refuse_moment(method, what):
    """The calls without method="moment" (`propagate` of the sparse classes, which spell it `propagate_moments`; the gradient
    chain of every class): ValueError naming them."""
    if method not in METHODS:
        raise ValueError(f"method must be 'linear' or 'moment', got {method!r}")
    if method == "moment":
        raise ValueError(f"method='moment' is not supported by {what}: the sparse classes serve exact moment matching through "
                         "predict_moments / propagate_moments, and the gradient through exact moments is "
                         "propagate_moments_gradient on every class")


def check_psd(S, what):
    """ValueError unless every matrix of S (.., n, n; symmetric) is positive semi-definite up to rounding (smallest eigenvalue >=
    -1e-12 of the largest entry).  The closed forms factor S + Lambda and R^-1 S: an indefinite S gives them a pivot that is not
    positive, and NaN or infinity without a message."""
    if S is not None and S.size and float(np.min(np.linalg.eigvalsh(S))) < -1e-12 * max(float(np.max(np.abs(S))), 1e-300):
        raise ValueError(f"{what} must be positive semi-definite")


def check_gaussian_queries(X, Sigma, D):
    """The arguments of `predict_moments` as contiguous float64 arrays: X (M, D) and Sigma (M, nx, nx) with nx <= D, the covariance
    of the leading nx coordinates of every query ((nx, nx): shared by all rows; None: zero, nx = D).  ValueError on a wrong shape,
    M outside 1 .. 32, NaN or infinity, a Sigma that is asymmetric or not positive semi-definite."""
    X = np.array(X, dtype=np.float64, ndmin=2)
    if X.ndim != 2 or X.shape[1] != D:
        raise ValueError(f"predict_moments: X must be (M, {D})")
    M = X.shape[0]
    if not (1 <= M <= MAX_R):
        raise ValueError(f"predict_moments: M must be in [1, {MAX_R}], got {M}")
    S = np.zeros((M, D, D)) if Sigma is None else np.asarray(Sigma, dtype=np.float64)
    if S.ndim == 2:
        S = np.broadcast_to(S, (M,) + S.shape)
    if S.ndim != 3 or S.shape[0] != M or S.shape[1] != S.shape[2] or not (1 <= S.shape[1] <= D):
        raise ValueError(f"predict_moments: Sigma must be (nx, nx) or ({M}, nx, nx) with nx <= {D}")
    if not (np.isfinite(X).all() and np.isfinite(S).all()):
        raise ValueError("predict_moments: X or Sigma contains NaN or infinity")
    if not np.array_equal(S, S.transpose(0, 2, 1)):
        raise ValueError("predict_moments: Sigma must be symmetric")
    check_psd(S, "predict_moments: Sigma")
    return np.ascontiguousarray(X), np.ascontiguousarray(S), M, S.shape[1]


def host_loop_moments(stage, coord, x0, U, lin, S0, Q, R, H):
    """The moment-matching recursion on the host.  stage(q (R, D) raw, Sigma (R, nx, nx)) -> (mean (R, NO), cov (R, NO, NO), xcov
    (R, NO, D) = Cov[q_d, y_o]) as `predict_moments` returns them; output o drives state coordinate coord[o]:

        x_{h+1}     = x_h + lin q + E mean
        Sigma_{h+1} = A0 Sigma_h A0^T + A0 Cx E^T + E Cx^T A0^T + E cov E^T + Q,       A0 = I + lin[:, :nx], Cx = xcov[:, :nx]^T

    Returns traj (H + 1, R, nx), Sigma (H + 1, R, nx, nx) and the stage quantities {"mean" (H, R, NO), "cov" (H, R, NO, NO), "xcov"
    (H, R, NO, D)}."""
    nx, D = lin.shape
    NO = len(coord)
    traj, Sigma = np.zeros((H + 1, R, nx)), np.zeros((H + 1, R, nx, nx))
    means, covs, xcovs = np.zeros((H, R, NO)), np.zeros((H, R, NO, NO)), np.zeros((H, R, NO, D))
    traj[0] = np.broadcast_to(x0, (R, nx))
    if S0 is not None:
        Sigma[0] = np.broadcast_to(S0, (R, nx, nx))
    A0 = np.eye(nx) + lin[:, :nx]
    E = np.zeros((nx, NO))
    for o, c in enumerate(coord):
        E[c, o] = 1.0
    for h in range(H):
        q = np.concatenate([traj[h], np.broadcast_to(U[:, h], (R, D - nx))], axis=1)
        mean, cov, xcov = stage(np.ascontiguousarray(q), np.ascontiguousarray(Sigma[h]))
        mean, cov, xcov = np.reshape(mean, (R, NO)), np.reshape(cov, (R, NO, NO)), np.reshape(xcov, (R, NO, D))
        means[h], covs[h], xcovs[h] = mean, cov, xcov
        F = A0 @ xcov[:, :, :nx].transpose(0, 2, 1) @ E.T       # A0 Cx E^T
        S = A0 @ Sigma[h] @ A0.T + F + F.transpose(0, 2, 1) + E @ cov @ E.T
        if Q is not None:
            S = S + Q
        traj[h + 1] = traj[h] + q @ lin.T + mean @ E.T
        Sigma[h + 1] = 0.5 * (S + S.transpose(0, 2, 1))
    return traj, Sigma, {"mean": means, "cov": covs, "xcov": xcovs}


def check_grad_order(order):
    """`propagate_gradient` differentiates the first-order propagation only: ValueError for any other order."""
    if isinstance(order, bool) or order != 1:
        raise ValueError(f"propagate_gradient: order must be 1, got {order!r} (the derivative of the second-order mean term "
                         "needs third derivatives of the mean, which the kernels do not form)")
    return 1


def check_seeds(grad_traj, grad_Sigma, R, H, nx):
    """The seeds as contiguous float64 arrays: gx (H + 1, R, nx) and gS (H + 1, R, nx, nx) or None.  With R = 1 the rollout
    axis may be left out.  ValueError on a wrong shape, NaN or infinity."""
    gx = np.asarray(grad_traj, dtype=np.float64)
    if gx.ndim == 2 and R == 1:
        gx = gx[:, None, :]
    if gx.shape != (H + 1, R, nx):
        raise ValueError(f"propagate_gradient: grad_traj must be ({H + 1}, {R}, {nx})" + (f" or ({H + 1}, {nx})" if R == 1 else ""))
    gS = None
    if grad_Sigma is not None:
        gS = np.asarray(grad_Sigma, dtype=np.float64)
        if gS.ndim == 3 and R == 1:
            gS = gS[:, None, :, :]
        if gS.shape != (H + 1, R, nx, nx):
            raise ValueError(f"propagate_gradient: grad_Sigma must be ({H + 1}, {R}, {nx}, {nx})"
                             + (f" or ({H + 1}, {nx}, {nx})" if R == 1 else ""))
    for name, a in (("grad_traj", gx), ("grad_Sigma", gS)):
        if a is not None and not np.isfinite(a).all():
            raise ValueError(f"propagate_gradient: {name} contains NaN or infinity")
    return np.ascontiguousarray(gx), (None if gS is None else np.ascontiguousarray(gS))


def _sym(a):
    """(a + a^T) / 2 over the last two axes, the lower triangle formed and mirrored: symmetric bit for bit"""
    low = np.tril(0.5 * (a + np.swapaxes(a, -1, -2)))
    return low + np.swapaxes(np.tril(low, -1), -1, -2)


def host_adjoint(stage, hess_stage, coord, x0, U, lin, S0, Q, R, H, gx, gS):
    """The forward recursion and the backward sweep of the module docstring on the host.  stage(q (R, D) raw) -> (mean (R, NO),
    jac (R, NO, D), var (R, NO), dvar (R, NO, D)), jac and dvar per unit of the raw query; hess_stage(q) -> the mean's Hessian
    (R, NO, D, D) per unit of the raw query.  Returns traj, Sigma (as `host_loop`), dU (R, H, nu), dx0 (R, nx), dSigma0 (R, nx,
    nx)."""
    nx, D = lin.shape
    NO = len(coord)
    kept = []

    def forward(q):
        mean, jac, var, dvar = stage(q)
        kept.append((q, np.asarray(jac).reshape(R, NO, D), np.asarray(dvar).reshape(R, NO, D)))
        return mean, jac, var

    traj, Sigma, _ = host_loop(forward, coord, x0, U, lin, S0, Q, R, H)
    lam = gx[H].copy()
    Lam = _sym(gS[H]) if gS is not None else np.zeros((R, nx, nx))
    dU = np.zeros((R, H, D - nx))
    F0 = np.concatenate([np.eye(nx), np.zeros((nx, D - nx))], axis=1) + lin
    for h in range(H - 1, -1, -1):
        q, jac, dvar = kept[h]
        hess = np.asarray(hess_stage(q)).reshape(R, NO, D, D)
        F = np.broadcast_to(F0, (R, nx, D)).copy()
        for o, c in enumerate(coord):
            F[:, c, :] += jac[:, o, :]
        A = F[:, :, :nx]
        G = Lam @ A @ Sigma[h]
        gq = np.einsum("rid,ri->rd", F, lam)
        for o, c in enumerate(coord):
            gq += Lam[:, c, c][:, None] * dvar[:, o, :] + 2.0 * np.einsum("rde,re->rd", hess[:, o, :, :nx], G[:, c, :])
        lam = gx[h] + gq[:, :nx]
        dU[:, h] = gq[:, nx:]
        Lam = A.transpose(0, 2, 1) @ Lam @ A
        if gS is not None:
            Lam = Lam + _sym(gS[h])
        Lam = _sym(Lam)
    return traj, Sigma, dU, lam, Lam


def check_moment_seeds(grad_mean, grad_cov, grad_xcov, M, NO, D):
    """The seeds of `predict_moments_vjp` as contiguous float64 arrays or None: grad_mean (M, NO), grad_cov (M, NO, NO), grad_xcov
    (M, NO, D); with M = 1 the leading axis may be left out.  ValueError on a wrong shape, NaN or infinity."""
    out = []
    for name, g, shape in (("grad_mean", grad_mean, (NO,)), ("grad_cov", grad_cov, (NO, NO)), ("grad_xcov", grad_xcov, (NO, D))):
        if g is not None:
            g = np.asarray(g, dtype=np.float64)
            if M == 1 and g.shape == shape:
                g = g[None]
            if g.shape != (M,) + shape:
                raise ValueError(f"predict_moments_vjp: {name} must be {(M,) + shape}")
            if not np.isfinite(g).all():
                raise ValueError(f"predict_moments_vjp: {name} contains NaN or infinity")
            g = np.ascontiguousarray(g)
        out.append(g)
    return tuple(out)


def host_adjoint_moments(stage, stage_vjp, coord, x0, U, lin, S0, Q, R, H, gx, gS):
    """The moment recursion (`host_loop_moments` over `stage`) and its backward sweep on the host.  stage_vjp(q (R, D) raw, Sigma
    (R, nx, nx), gmean (R, NO), gcov (R, NO, NO), gxcov (R, NO, D)) -> (.., dq (R, D), dSigma (R, nx, nx)) as `predict_moments_vjp`
    returns them (its last two results are read).  Returns traj, Sigma (as `host_loop_moments`), dU (R, H, nu), dx0 (R, nx),
    dSigma0 (R, nx, nx)."""
    nx, D = lin.shape
    NO = len(coord)
    traj, Sigma, _ = host_loop_moments(stage, coord, x0, U, lin, S0, Q, R, H)
    A0 = np.eye(nx) + lin[:, :nx]
    E = np.zeros((nx, NO))
    for o, c in enumerate(coord):
        E[c, o] = 1.0
    F0 = np.concatenate([np.eye(nx), np.zeros((nx, D - nx))], axis=1) + lin
    lam = gx[H].copy()
    Lam = _sym(gS[H]) if gS is not None else np.zeros((R, nx, nx))
    dU = np.zeros((R, H, D - nx))
    for h in range(H - 1, -1, -1):
        q = np.ascontiguousarray(np.concatenate([traj[h], np.broadcast_to(U[:, h], (R, D - nx))], axis=1))
        gxcov = np.zeros((R, NO, D))
        gxcov[:, :, :nx] = 2.0 * (E.T @ Lam @ A0)
        out = stage_vjp(q, np.ascontiguousarray(Sigma[h]), np.ascontiguousarray(lam @ E), np.ascontiguousarray(E.T @ Lam @ E), gxcov)
        dq, dS = np.reshape(out[-2], (R, D)), np.reshape(out[-1], (R, nx, nx))
        gq = lam @ F0 + dq
        lam = gx[h] + gq[:, :nx]
        dU[:, h] = gq[:, nx:]
        Lam = A0.T @ Lam @ A0 + dS
        if gS is not None:
            Lam = Lam + _sym(gS[h])
        Lam = _sym(Lam)
    return traj, Sigma, dU, lam, Lam


def nominal_adjoint(lin, R, H, gx, gS):
    """The sweep through the nominal dynamics alone (A = I + lin_x, F = [I 0] + lin, no variance terms): the wrappers'
    fallback.  Returns dU (R, H, nu), dx0 (R, nx)."""
    nx, D = lin.shape
    F = np.concatenate([np.eye(nx), np.zeros((nx, D - nx))], axis=1) + lin
    lam = gx[H].copy()
    dU = np.zeros((R, H, D - nx))
    for h in range(H - 1, -1, -1):
        gq = lam @ F
        lam = gx[h] + gq[:, :nx]
        dU[:, h] = gq[:, nx:]
    return dU, lam


# ---- what the batches (BatchedARDGP, BatchedSparseGP) share: raw units around single-output models --------------------------------
def check_route(route, routes=("auto", "host")):
    """ValueError unless `route` is one of `routes` (the sparse classes add "chain", the one-call device chain)."""
    if route not in routes:
        raise ValueError("route must be " + " or ".join(repr(r) for r in routes))
    return route


def wrapper_route(model):
    """The route a control-loop wrapper asks of its model: the sparse classes' one-call chain where their predicate
    `propagate_ok()` holds, otherwise "auto" (the exact classes choose by themselves; the sparse ones run the host loop)."""
    ok = getattr(model, "propagate_ok", None)
    return "chain" if callable(ok) and ok() else "auto"


def model_horizon(model, x0, U, lin, order=1, method="linear", **kw):
    """The horizon a control-loop wrapper asks of its model -> (traj, Sigma).  method="moment": `propagate_moments` of a sparse
    class (its one-call chain; the model is assembled, and its Q formed, from the rows it has taken so far), `propagate(method=
    "moment")` of an exact one; otherwise `propagate` on the `wrapper_route`.  kw: Sigma0, process_noise and, for a batch,
    coord and the scalers."""
    if method == "moment" and callable(getattr(model, "propagate_moments", None)):
        return model.propagate_moments(x0, U, lin, **kw)
    return model.propagate(x0, U, lin, route=wrapper_route(model), order=order, method=method, **kw)


def model_moments_gradient(model, x0, U, lin, grad_traj, grad_Sigma, **kw):
    """The gradient through exact moments that a control-loop wrapper asks of its model: `propagate_moments_gradient`, on its
    default route (an exact class: one call; a sparse class: its one-call chain, the model assembled and its Q formed from the rows
    it has taken so far).  ValueError "<class> has no gradient through exact moments", with the reason, for a class without the
    method and for a model that cannot serve the call: not fitted, no inducing inputs, attributes missing.  kw: for a batch,
    coord and the scalers."""
    name = type(model).__name__
    fn = getattr(model, "propagate_moments_gradient", None)
    if not callable(fn):
        raise ValueError(f"{name} has no gradient through exact moments (it has no method propagate_moments_gradient)")
    try:
        return fn(x0, U, lin, grad_traj, grad_Sigma, **kw)
    except AttributeError as e:
        raise ValueError(f"{name} has no gradient through exact moments: the model is not fitted ({e})") from None
    except RuntimeError as e:
        if isinstance(e, _lib.GPKError):      # the library's own failures are not the model's state
            raise
        raise ValueError(f"{name} has no gradient through exact moments: {e}") from None


def chain_sizes_ok(m, D, nx):
    """The sizes within the limits of gpk_sparse_propagate[_multi]: m inducing points (padded to 128) <= 16 384,
    1 <= nx <= D <= 16.  Returns the reason as a string where they are not, None where they are."""
    if not (1 <= nx <= D <= 16):
        return f"the chain needs 1 <= nx <= D <= 16 (nx = {nx}, D = {D})"
    if -(-int(m) // 128) * 128 > 16384:
        return f"the chain needs at most 16384 inducing points after padding (m = {m})"
    return None


def check_batch(B, D, x0, U, lin, coord, in_scaler, out_scaler, Sigma0, process_noise, route, routes=("auto", "host")):
    """The arguments of a batch's `propagate`: `check_horizon`'s results, then coord (list), in_shift, in_scale ((D,) or None),
    o_mean, o_scale ((B,): the identity without an out_scaler).  routes: what the class accepts for `route`."""
    lin = np.asarray(lin, dtype=np.float64)
    nx = lin.shape[0] if lin.ndim == 2 else 0
    if not (B <= nx <= D):
        raise ValueError(f"propagate needs a state of {B} <= nx <= {D} coordinates (got {nx})")
    check_route(route, routes)
    head = check_horizon(x0, U, lin, nx, D, Sigma0, process_noise)
    coord = check_coord(coord, B, nx)
    return head + (coord,) + check_scalers(B, D, in_scaler, out_scaler)


def check_scalers(B, D, in_scaler, out_scaler):
    """A batch's scalers: in_shift, in_scale ((D,) or None), o_mean, o_scale ((B,): the identity without an out_scaler)."""
    in_shift = in_scale = None
    if in_scaler is not None:
        pair = (in_scaler.mean_, in_scaler.scale_) if hasattr(in_scaler, "mean_") else in_scaler
        in_shift = np.ascontiguousarray(np.broadcast_to(np.asarray(pair[0], dtype=np.float64), (D,)))
        in_scale = np.ascontiguousarray(np.broadcast_to(np.asarray(pair[1], dtype=np.float64), (D,)))
        if not (np.isfinite(in_shift).all() and np.isfinite(in_scale).all()):
            raise ValueError("the input scaler contains NaN or infinity.")
        if not in_scale.all():
            raise ValueError("in_scale must be non-zero")
    o_mean, o_scale = np.zeros(B), np.ones(B)
    if out_scaler is not None:
        o_mean = np.broadcast_to(np.asarray(out_scaler[0], dtype=np.float64), (B,))
        o_scale = np.broadcast_to(np.asarray(out_scaler[1], dtype=np.float64), (B,))
        if not (np.isfinite(o_mean).all() and np.isfinite(o_scale).all()):
            raise ValueError("the output scaler contains NaN or infinity.")
    return in_shift, in_scale, o_mean, o_scale


def batch_stage(predict_jacobian, level, in_shift, in_scale, o_mean, o_scale, var_includes_noise, with_dvar=False):
    """The `host_loop` stage of a batch: predict_jacobian(z, return_var=True) -> (mean (R, B), dmean (R, B, D), var (R, B), dvar
    (R, B, D)) on the scaled rows; level (B,): the noise level's share of every model's variance, which the served variances
    carry.  with_dvar: the stage of `host_adjoint`, with the variance gradient per unit of the raw query as its fourth result."""
    def stage(q):
        z = q if in_shift is None else (q - in_shift) / in_scale
        mean, dmean, var, dvar = predict_jacobian(z, return_var=True)
        if not var_includes_noise:      # the latent variance, clipped again
            var = np.maximum(var - level[None, :], 0.0)
        if in_scale is not None:
            dmean = dmean / in_scale[None, None, :]
        head = (o_mean + o_scale * mean, o_scale[None, :, None] * dmean, o_scale ** 2 * var)
        if not with_dvar:
            return head
        if in_scale is not None:
            dvar = dvar / in_scale[None, None, :]
        return head + ((o_scale ** 2)[None, :, None] * dvar,)

    return stage


def batch_hess_stage(predict_hessian, in_shift, in_scale, o_scale):
    """The second-order `host_loop` stage of a batch: predict_hessian(z) -> (_, _, hess (R, B, D, D)) on the scaled rows, returned
    per unit of the raw query and behind the output scaler, as `batch_stage` returns the Jacobian."""
    def hess_stage(q):
        z = q if in_shift is None else (q - in_shift) / in_scale
        hess = predict_hessian(z)[2]
        if in_scale is not None:
            hess = hess / (in_scale[None, None, :, None] * in_scale[None, None, None, :])
        return o_scale[None, :, None, None] * hess

    return hess_stage


def noise_levels(models):
    """noise level times y_std^2 of single-output models: what `var_includes_noise=False` takes off the served variances"""
    return np.array([(m.kernel_.components().noise or 0.0) * float(np.ravel(m._y_train_std)[0]) ** 2 for m in models])


# ---- the control-loop wrappers (SimpleQuadrotorGP / PreTrainedGP .propagate_horizon): 6 states, 4 controls ------------------------
def horizon_inputs(dynamics, state, U_guess, dt):
    """state (6,), U_guess (4+, N) or (R, 4+, N) -> (state, U (R, N, 4), lin (6, 10), nominal trajectory (N + 1, R, 6), single):
    `lin` and the nominal trajectory of `dynamics` as `paths.nominal_rollouts` gives them."""
    from .paths import nominal_rollouts
    state = np.asarray(state, dtype=float).reshape(-1)[:6]
    U_guess = np.asarray(U_guess, dtype=float)
    single = U_guess.ndim == 2
    Ug = U_guess[None] if single else U_guess
    noms = [nominal_rollouts(dynamics, state, Ug[r], dt, 1) for r in range(Ug.shape[0])]
    nominal = np.stack([n[0][0] for n in noms], axis=0).transpose(2, 0, 1)
    return state, np.ascontiguousarray(Ug[:, :4, :].transpose(0, 2, 1)), noms[0][1], nominal, single


def horizon_layout(traj, Sigma, single):
    """traj (N + 1, R, 6), Sigma (N + 1, R, 6, 6) -> the trainers' layout X (R, 6, N + 1), Sigma (R, N + 1, 6, 6); `single`
    drops R."""
    X, S = np.ascontiguousarray(traj.transpose(1, 2, 0)), np.ascontiguousarray(Sigma.transpose(1, 0, 2, 3))
    return (X[0], S[0]) if single else (X, S)


def nominal_horizon(nominal, lin, Sigma0, process_noise):
    """The fallback of the wrappers: the nominal trajectory with Sigma_{k+1} = (I + lin_x) Sigma_k (I + lin_x)^T + Q; arguments
    that cannot be read as (6, 6) count as zero (it must not raise)."""
    H, R, nx = nominal.shape[0] - 1, nominal.shape[1], nominal.shape[2]

    def mat(a):
        try:
            a = np.zeros((nx, nx)) if a is None else np.asarray(a, dtype=float)
            return a if a.shape[-2:] == (nx, nx) and a.ndim in (2, 3) and np.isfinite(a).all() else np.zeros((nx, nx))
        except Exception:  # noqa: BLE001
            return np.zeros((nx, nx))

    S0, Q = mat(Sigma0), mat(process_noise)
    if Q.ndim != 2:
        Q = np.zeros((nx, nx))
    A = np.eye(nx) + lin[:, :nx]
    Sigma = np.empty((H + 1, R, nx, nx))
    Sigma[0] = S0
    for k in range(H):
        Sigma[k + 1] = A @ Sigma[k] @ A.T + Q
    return nominal, Sigma


def gradient_layout(traj, Sigma, dU, dx0, single):
    """`horizon_layout` for the wrappers' `horizon_gradient`: X, Sigma as there, dU (R, N, nu), dx0 (R, 6); `single` drops R."""
    X, S = horizon_layout(traj, Sigma, single)
    return (X, S, dU[0], dx0[0]) if single else (X, S, dU, dx0)


def nominal_gradient(nominal, lin, grad_traj, single):
    """The fallback of the wrappers' `horizon_gradient`: the nominal horizon (zero covariance) and the sweep through the nominal
    dynamics; seeds that cannot be read as (N + 1, R, 6) count as zero (it must not raise)."""
    H, R, nx = nominal.shape[0] - 1, nominal.shape[1], nominal.shape[2]
    try:
        gx, _ = check_seeds(grad_traj, None, R, H, nx)
    except Exception:  # noqa: BLE001
        gx = np.zeros((H + 1, R, nx))
    dU, dx0 = nominal_adjoint(lin, R, H, gx, None)
    return gradient_layout(*nominal_horizon(nominal, lin, None, None), dU, dx0, single)
