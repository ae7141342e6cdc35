"""CPU pins of the QP checkers (oracle.qp_exact_general, oracle.qp_exact) on
degenerate problems: dependent, duplicate, parallel and antiparallel rows,
more than n tight rows, tight rows with a zero multiplier, infeasible pairs.

The optimum is known by construction (tests/_qp_cases.py), so the oracle is
checked against z* itself: status 0 everywhere and z within 1e-9 of z*
relative to max(1, |z*|) (<= 1e-13 observed on the dyadic families); within
1e-8 on the fp64-only families 'near' and 'illcond', a factor 10 inside the
1e-7 bar the kernels are held to on them.

qp_exact_general used to accept an active-set guess with linearly dependent
rows whenever the computed determinant of its singular KKT matrix was not
exactly 0 (~1e-15): multipliers ~1e16 and a z that is feasible but not
stationary.  test_dependent_rows_explicit_case is such a QP by value.
"""
import numpy as np
import pytest

import _qp_cases as C
from oracle import oracle as O


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def test_dependent_rows_explicit_case():
    P = np.array([[[7.0, 2.0], [2.0, 6.0]]]); q = np.array([[-9.5, 2.0]])
    G = np.array([[[1.0, 1.0], [-3.0, -3.0], [0.0, 1.0], [2.0, 2.0]]]); h = np.array([[0.25, 0.75, -1.25, 2.5]])
    z_star = np.array([[1.5, -1.25]]); lam_star = np.array([[1.5, 0.0, 1.0, 0.0]])
    # the constructed point satisfies KKT exactly
    r = C.kkt_residuals(P, q, G, h, z_star, lam_star)
    assert r == dict(dual=0.0, primal=0.0, stationarity=0.0, complementarity=0.0)
    z, lam, act, st = O.qp_exact_general(P, q, G, h)
    assert st[0] == 0
    assert rel(z, z_star) <= 1e-9
    assert np.isfinite(lam).all() and lam.max() < 1e3
    r = C.kkt_residuals(P, q, G, h, z, lam)
    assert max(r.values()) <= 1e-9


@pytest.mark.parametrize("n,m", C.SHAPES)
def test_oracle_recovers_constructed_optimum(n, m):
    rng = np.random.default_rng(1000 * n + m)
    B = 24
    for fam in C.FEASIBLE:
        d = C.kkt_qps(rng, B, n, m, fam)
        r = C.kkt_residuals(d["P"], d["q"], d["G"], d["h"], d["z"], d["lam"])
        assert max(r.values()) <= (1e-8 if fam in C.FP64_ONLY else 0.0), (fam, r)   # the construction itself
        z, lam, act, st = O.qp_exact_general(d["P"], d["q"], d["G"], d["h"])
        assert (st == 0).all(), fam
        # 'near' and 'illcond': a factor 10 inside their 1e-7 bar on the GPU
        assert rel(z, d["z"]) <= (1e-8 if fam in C.FP64_ONLY else 1e-9), fam
        assert np.isfinite(lam).all() and (lam >= 0).all(), fam


@pytest.mark.parametrize("n,m", C.SHAPES)
def test_qp_exact_on_the_diagonal_family(n, m):
    """qp_exact takes q = 0: the constructed QP is shifted to it (z = y - c
    with P c = q turns 1/2 y'Py + q'y into 1/2 z'Pz + const, rows G z <= h + G c)."""
    rng = np.random.default_rng(2000 * n + m)
    d = C.kkt_qps(rng, 24, n, m, "diag")
    Pd = np.einsum("bkk->bk", d["P"])
    c = d["q"] / Pd
    z, lam, act, st = O.qp_exact(Pd, d["G"], d["h"] + np.einsum("bmn,bn->bm", d["G"], c))
    assert (st == 0).all()
    assert rel(z - c, d["z"]) <= 1e-9


@pytest.mark.parametrize("n,m", [s for s in C.SHAPES if s[1] >= 2])
def test_infeasible_family_is_reported(n, m):
    rng = np.random.default_rng(3000 * n + m)
    d = C.kkt_qps(rng, 24, n, m, "infeasible")
    st = O.qp_exact_general(d["P"], d["q"], d["G"], d["h"])[3]
    assert (st == 2).all()
    Pd = np.ones((24, n))
    assert (O.qp_exact(Pd, d["G"], d["h"])[3] == 2).all()


def test_case_generator_families_are_what_they_say():
    """The degenerate families are degenerate: tight rows beyond the
    multipliers' support, exact duplicates, (anti)parallel pairs."""
    rng = np.random.default_rng(5)
    n, m, B = 2, 8, 64
    tight = lambda d: np.abs(d["h"] - np.einsum("bmn,bn->bm", d["G"], d["z"])) == 0.0
    d = C.kkt_qps(rng, B, n, m, "full")
    assert (tight(d) == (d["lam"] > 0)).all()
    d = C.kkt_qps(rng, B, n, m, "weak")
    assert ((tight(d) & (d["lam"] == 0)).sum(axis=1) == 1).all()
    d = C.kkt_qps(rng, B, n, m, "vertex")
    assert (tight(d).sum(axis=1) == n + 2).all()
    cross = lambda G: G[:, :, None, 0] * G[:, None, :, 1] - G[:, :, None, 1] * G[:, None, :, 0]
    dot = lambda G: np.einsum("bik,bjk->bij", G, G)
    off = ~np.eye(m, dtype=bool)[None]
    d = C.kkt_qps(rng, B, n, m, "dup")
    Gh = np.concatenate([d["G"], d["h"][..., None]], -1)
    assert (((Gh[:, :, None] == Gh[:, None, :]).all(-1) & off).any(axis=(1, 2))).all()
    d = C.kkt_qps(rng, B, n, m, "parallel")
    assert (((cross(d["G"]) == 0) & (dot(d["G"]) > 0) & off).any(axis=(1, 2))).all()
    for fam in ("antiparallel_feasible", "infeasible"):
        d = C.kkt_qps(rng, B, n, m, fam)
        assert (((d["G"][:, :, None] == -d["G"][:, None, :]).all(-1)).any(axis=(1, 2))).all()
    d = C.kkt_qps(rng, B, n, m, "diag")
    assert (d["P"] == d["P"] * np.eye(n)).all()
