"""Writes tests/golden/sparse_select_ref.npz: greedy conditional-variance selection of inducing inputs ("choosing
Z"; Burt, Rasmussen, van der Wilk, JMLR 2020), the pivoted partial Cholesky factorisation of Kff that never forms Kff.

NumPy only, seeded, reproduces its file bit for bit: every sum of the recursion is a loop of elementwise operations in a fixed
order (no BLAS call whose blocking could differ).  Three functions are the reference of the GPU tests:

* `greedy_select(X, ls, sf2, m_max, min_var, tol)`: the algorithm as include/gpk.h states it (gpk_greedy_select);
* `follow(X, ls, sf2, idx)`: the same recursion along a GIVEN index sequence; returns every step's full d (before the step) and
  trace (after it) - what judges a sequence where ties are real and no fixed sequence exists;
* `dense_trace(X, ls, sf2, idx)`: tr(Kff - Kfu Kuu^-1 Kuf) by a Cholesky factorisation of Kuu, an independent form.

The three stored cases are tie-free: X = standard normal (n, D), ls = exp(U(lo, hi)) per feature, sf2 = 1.7.  At every step
after the first the gap between the largest and the second-largest d is at least GAP_GATE sf2 = 1e-8 sf2 (asserted; the smallest
gap is stored), while the recursion's rounding error in d is about t eps sf2 <= 1e-12 sf2: four orders under the gap, which is
what makes an exact comparison of the indices legitimate.  (At the first step every d equals sf2 and the lowest index wins.)

    python tests/golden/make_golden_sparse_select.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sparse_select_ref.npz")

SF2 = 1.7
GAP_GATE = 1e-8
SEED = 0
# name: (n, D, m, lo, hi)
CASES = {"A": (600, 2, 64, 0.0, 0.6), "B": (1500, 3, 130, 0.2, 0.8), "C": (2100, 4, 200, 0.4, 1.0)}


def kernel_column(X, ls, sf2, j):
    """sf2 exp(-1/2 sum_d (x_id / ls_d - x_jd / ls_d)^2): exact differences of the divided coordinates, features in order"""
    Xs = X / ls
    q = np.zeros(X.shape[0])
    for d in range(X.shape[1]):
        e = Xs[:, d] - Xs[j, d]
        q += e * e
    return sf2 * np.exp(-0.5 * q)


def _step(X, ls, sf2, Lt, t, j, d):
    """One step at pivot j: the new panel column (stored as row t of Lt) and d, in place."""
    acc = np.zeros(X.shape[0])
    for s in range(t):
        acc += Lt[s] * Lt[s, j]
    l = (kernel_column(X, ls, sf2, j) - acc) / np.sqrt(d[j])
    Lt[t] = l
    np.maximum(d - l * l, 0.0, out=d)
    d[j] = 0.0


def greedy_select(X, ls, sf2, m_max, min_var=1e-10, tol=0.0, gaps=None):
    """Returns (idx, trace, dmax), each of `selected` entries.  gaps (a list): receives, per step, largest minus second-largest d."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    d = np.full(n, float(sf2))
    Lt = np.zeros((m_max, n))
    idx, trace, dmax = [], [], []
    t = 0
    while True:
        j = int(np.argmax(d))        # the first of the largest: the lowest index
        if t == m_max or d[j] <= min_var * sf2 or (t >= 1 and d.sum() <= tol * n * sf2):
            break
        if gaps is not None and n > 1:
            top = np.partition(d, n - 2)[n - 2:]
            gaps.append(float(top[1] - top[0]))
        idx.append(j)
        dmax.append(float(d[j]))
        _step(X, ls, sf2, Lt, t, j, d)
        trace.append(float(d.sum()))
        t += 1
    return np.array(idx, dtype=np.int64), np.array(trace), np.array(dmax)


def follow(X, ls, sf2, idx):
    """The recursion along idx.  Returns (d_before (T, n): the full d that step t chose from, trace (T,): sum of d after step t)."""
    X = np.asarray(X, dtype=np.float64)
    n, T = X.shape[0], len(idx)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    d = np.full(n, float(sf2))
    Lt = np.zeros((T, n))
    d_before, trace = np.empty((T, n)), np.empty(T)
    for t, j in enumerate(idx):
        d_before[t] = d
        _step(X, ls, sf2, Lt, t, int(j), d)
        trace[t] = d.sum()
    return d_before, trace


def dense_trace(X, ls, sf2, idx):
    """tr(Kff - Kfu Kuu^-1 Kuf) with Z = X[idx]: n sf2 - |Luu^-1 Kuf|_F^2"""
    X = np.asarray(X, dtype=np.float64)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X.shape[1],))
    Kuf = np.stack([kernel_column(X, ls, sf2, int(j)) for j in idx])
    Kuu = Kuf[:, np.asarray(idx, dtype=np.int64)]
    V = np.linalg.solve(np.linalg.cholesky(Kuu), Kuf)
    return X.shape[0] * sf2 - float(np.sum(V * V))


def make_case(n, D, lo, hi, seed=SEED):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D))
    ls = np.exp(rng.uniform(lo, hi, D))
    return X, ls


def build():
    out = {"sf2": np.float64(SF2), "gap_gate": np.float64(GAP_GATE)}
    for name, (n, D, m, lo, hi) in CASES.items():
        X, ls = make_case(n, D, lo, hi)
        gaps = []
        idx, trace, dmax = greedy_select(X, ls, SF2, m, gaps=gaps)
        assert len(idx) == m, f"case {name}: stopped after {len(idx)} of {m}"
        gap = min(gaps[1:])
        assert gap >= GAP_GATE * SF2, f"case {name}: gap {gap:.2e} under {GAP_GATE * SF2:.1e}: pick another seed"
        dense = dense_trace(X, ls, SF2, idx)
        assert abs(dense - trace[-1]) <= 1e-9 * n * SF2
        out.update({f"{name}_X": X, f"{name}_ls": ls, f"{name}_idx": idx, f"{name}_trace": trace, f"{name}_dmax": dmax,
                    f"{name}_min_gap": np.float64(gap), f"{name}_dense_last": np.float64(dense)})
        print(f"case {name}: n {n} D {D} m {m}: smallest gap {gap:.2e}, trace / (n sf2) {trace[-1] / (n * SF2):.3e}, "
              f"dense form differs by {abs(dense - trace[-1]) / (n * SF2):.1e} n sf2")
    return out


if __name__ == "__main__":
    np.savez(OUT, **build())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
