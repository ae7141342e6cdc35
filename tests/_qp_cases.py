"""QPs whose optimum is known by construction, for the generic QP kernels
(rcbf_qp_solve and its kin) and for the oracle that checks them.

kkt_qps builds   min 1/2 z'Pz + q'z  s.t.  G z <= h   backwards from its KKT
point: choose z*, the rows with a positive multiplier (at most min(n, m),
linearly independent), lam* >= 0 and a slack >= 0 for every other row, then
h = G z* + slack and q = -(P z* + G' lam*).  P is SPD, so z* is the unique
optimum and needs no solver to certify it.

The dyadic families (DYADIC) use small dyadic data -- P = A A' + n I with
integer A (a positive integer diagonal for 'diag'), integer rows in [-3, 3]
with no zero row, z*, lam* and slacks multiples of 1/4 -- so P, q, G, h are
exact in fp32 (asserted) and the fp32 and fp64 entry points get the same QP:

  full      dense P, strictly complementary (every slack and multiplier > 0)
  diag      the same with a diagonal P
  weak      one extra tight row with lam* = 0
  vertex    up to n + 2 rows tight at z*, as many as m allows
  dup       a row repeated exactly (tight, with lam* = 0, where its source is tight)
  parallel  twice a row, with a looser, an equal or a tighter h; when the
            new row is the tighter one it is the tight one
  antiparallel_feasible   a row and its negative: a slab that contains z*;
            one side may be tight
  infeasible              a row, and its negative with h' = -h - 1 (no z*)

Two further families are fp64 only, their data not dyadic (FP64_ONLY).  Their
rows are integer rows in [-1, 1]: the oracle's own error on them grows with
the rows' size, and it has to stay a factor 10 inside the 1e-7 bar the fp64
kernels are held to on them.

  near      dense P; slacks in {1e-6, 1e-9, 1e-11}, positive multipliers in
            {1e-6, 1e-9}, and a near-parallel pair G_d = G_s + delta e_k, both
            tight.  delta = NEAR_DELTA = 1e-3.  The oracle accepts a candidate
            whose rows are violated by tol * scale (~1e-9), so it may leave
            out a row whose multiplier is 1e-9: measured over every shape of
            SHAPES at B = 300, raw and normalised rows, it is within 6.7e-9
            of z* (relative to max(1, |z*|)); the multipliers, not delta, set
            that figure (1.3e-8 with rows in [-3, 3] at delta = 1e-4 and 1e-3
            alike).
  illcond   diagonal P spanning the project's own extremes, (1, 1e-2, 1e5)
            and (10, 1e-4, 1e7) (the first n entries), otherwise as 'weak',
            with z*_k scaled by 1 / max(1, P_kk) and multipliers <= 1 so
            that q stays O(1).  The oracle is within 1.1e-15 of z*.  (With
            z* = O(1) on the heavy coordinate q is ~1e7, the oracle's
            absolute tolerance tol * (1 + |q|) admits a wrong active set and
            it is 8e-6 off: that variant was dropped.)
"""
import itertools

import numpy as np

DYADIC = ("full", "diag", "weak", "vertex", "dup", "parallel", "antiparallel_feasible")
FP64_ONLY = ("near", "illcond")
FEASIBLE = DYADIC + FP64_ONLY
FAMILIES = FEASIBLE + ("infeasible",)
NEAR_DELTA = 1e-3
ILLCOND_P = ((1.0, 1e-2, 1e5), (10.0, 1e-4, 1e7))

NS = (1, 2, 3)
MS = (1, 4, 5, 8, 9, 12, 13, 16)
SHAPES = tuple((n, m) for n in NS for m in MS) + ((3, 7),)


def _quarters(rng, lo, hi, size=None):
    """Multiples of 1/4 in [lo, hi]."""
    return rng.integers(int(lo * 4), int(hi * 4) + 1, size) / 4.0


def _row(rng, n, amax=3):
    """A non-zero integer row with entries in [-amax, amax]."""
    while True:
        g = rng.integers(-amax, amax + 1, n).astype(np.float64)
        if g.any():
            return g


def _independent_rows(rng, k, n, first_amax=3, amax=3):
    """k linearly independent integer rows (row 0 within first_amax, the
    others within amax)."""
    while True:
        R = np.stack([_row(rng, n, first_amax if i == 0 else amax) for i in range(k)]) if k else np.zeros((0, n))
        if k == 0 or np.linalg.matrix_rank(R) == k:
            return R


def _has_interior(Gt):
    """Is there a d with Gt d < 0 (a feasible direction off every tight row)?
    By Gordan's theorem, iff no y >= 0, y != 0 has Gt' y = 0; by Caratheodory
    such a y can be taken on a minimal dependent subset of <= n + 1 rows."""
    t, n = Gt.shape
    for s in range(2, min(t, n + 1) + 1):
        for S in itertools.combinations(range(t), s):
            u, sv, vt = np.linalg.svd(Gt[list(S)].T)          # null space of Gt_S'
            if (sv > 1e-9).sum() != s - 1:
                continue
            y = vt[-1]
            if (y >= -1e-9).all() or (y <= 1e-9).all():
                return False
    return True


def _one(rng, n, m, family):
    """One QP whose feasible set has an interior (see kkt_qps)."""
    while True:
        P, q, G, h, z, lam, slack = _draw(rng, n, m, family)
        if family == "infeasible" or _has_interior(G[slack == 0.0]):
            return P, q, G, h, z, lam


def _draw(rng, n, m, family):
    """One QP: P, q, G, h, z*, lam* (z* is NaN for 'infeasible') and the slacks."""
    dense = family not in ("diag", "illcond")
    if family == "illcond":
        P = np.diag(np.array(ILLCOND_P[rng.integers(0, 2)])[:n])
    elif dense:
        A = rng.integers(-2, 3, (n, n)).astype(np.float64)
        P = A @ A.T + n * np.eye(n)
    else:
        P = np.diag(rng.integers(1, 9, n).astype(np.float64))
    z = _quarters(rng, -2, 2, n)
    if family == "illcond":
        # as in the project's own ill-conditioned QP (the Cascade unicycle's, q = 0), a heavily weighted
        # coordinate is small at the optimum: |P z*| and so |q| stay O(1).  With z* = O(1) there q is ~1e7
        # and the oracle's absolute tolerance tol * (1 + |q|) admits a wrong active set (8e-6 off z*).
        z = z / np.maximum(1.0, np.diagonal(P))
    # the rows with a positive multiplier come first while the QP is built; a
    # permutation at the end spreads them over the m positions
    pair = family in ("dup", "parallel", "antiparallel_feasible", "infeasible", "near") and m >= 2
    extra = 1 if (pair or family in ("weak", "illcond")) else 0   # a row this family adds besides the active ones
    kmax = max(0, min(n, m - extra))
    k = int(rng.integers(1 if kmax else 0, kmax + 1))
    if rng.random() < 0.125:
        k = 0                              # now and then no row carries a multiplier
    small_first = family == "parallel"
    # the fp64-only families keep their rows in [-1, 1]: the oracle's own error on them grows with |g|
    amax = 1 if family in FP64_ONLY else 3
    G = np.zeros((m, n)); slack = np.zeros(m); lam = np.zeros(m)
    G[:k] = _independent_rows(rng, k, n, 1 if small_first else amax, amax)
    for r in range(k, m):
        G[r] = _row(rng, n, 1 if (small_first and r == 0) else amax)
    if family == "near":
        lam[:k] = rng.choice([1e-6, 1e-9], k)
        slack[k:] = rng.choice([1e-6, 1e-9, 1e-11], m - k)
    else:
        # 'illcond': multipliers <= 1 keep |q|, and with it the oracle's absolute tolerance, small
        lam[:k] = _quarters(rng, 0.25, 1 if family == "illcond" else 3, k)
        slack[k:] = _quarters(rng, 0.25, 3, m - k)
    if family in ("weak", "illcond"):
        if k < m:
            slack[k] = 0.0
    elif family == "vertex":
        slack[k:min(m, n + 2)] = 0.0
    src, d = 0, max(k, 1)   # the pair: row 0 (active when k >= 1) and the first row after the active ones
    scale_h = None
    if pair:
        if family == "dup":
            G[d] = G[src]; slack[d] = slack[src]
        elif family == "parallel":
            kind = rng.integers(0, 3)      # looser, equal, tighter
            G[d] = G[src]
            if kind == 2:                  # the doubled row is the tight (active) one, the plain row is loose
                G[src] = 2.0 * G[src]
                slack[d] = _quarters(rng, 0.25, 3)
            else:
                scale_h = (d, 2.0)
                slack[d] = 0.0 if kind == 1 else _quarters(rng, 0.25, 3)
                slack[d] += slack[src]
        elif family == "antiparallel_feasible":
            G[d] = -G[src]
            slack[d] = _quarters(rng, 0.25, 3) if (slack[src] == 0.0 or rng.random() < 0.5) else 0.0
        elif family == "infeasible":
            G[d] = -G[src]
        elif family == "near":
            G[d] = G[src]; G[d, rng.integers(0, n)] += NEAR_DELTA
            slack[d] = 0.0
            if k == 0:
                slack[src] = 0.0
    h = G @ z + slack
    if scale_h is not None:                # row d = 2 * row src:  2 g z <= 2 (g z* + slack)
        r, c = scale_h
        G[r] *= c; h[r] *= c; slack[r] *= c
    if family == "infeasible" and pair:
        h[d] = -h[src] - 1.0
    q = -(P @ z + G.T @ lam)
    perm = rng.permutation(m)
    G, h, lam, slack = G[perm], h[perm], lam[perm], slack[perm]
    if family == "infeasible":
        z = np.full(n, np.nan)
    return P, q, G, h, z, lam, slack


def kkt_qps(rng, B, n, m, family):
    """B QPs of one family: dict of P (B,n,n), q (B,n), G (B,m,n), h (B,m),
    z (B,n) the constructed optimum and lam (B,m) its multipliers, all fp64.
    'infeasible' needs m >= 2.

    A draw whose tight rows admit no common strictly feasible direction (a
    positive combination of them vanishes, e.g. both sides of a zero-width
    slab, or three tight rows around a point in the plane) is drawn again:
    its feasible set has no interior, so the rounding of the row normaliser
    (G / N, h / N in fp32 or fp64) can leave it empty, and then no reference
    exists -- the oracle rightly reports such a normalised QP infeasible."""
    assert family in FAMILIES, family
    assert family != "infeasible" or m >= 2
    parts = [_one(rng, n, m, family) for _ in range(B)]
    out = {k: np.stack([p[i] for p in parts]) for i, k in enumerate(("P", "q", "G", "h", "z", "lam"))}
    if family not in FP64_ONLY:
        for k in ("P", "q", "G", "h"):
            assert np.array_equal(out[k].astype(np.float32).astype(np.float64), out[k]), (family, k)
        assert np.abs(out["G"]).max() <= 3 and (np.abs(out["G"]).max(axis=2) > 0).all()
    return out


def kkt_residuals(P, q, G, h, z, lam):
    """The four KKT residuals of (z, lam), the worst over the batch:
    -min(lam), max(G z - h), max |P z + q + G' lam|, max |lam (h - G z)|."""
    P, q, G, h, z, lam = (np.asarray(a, np.float64) for a in (P, q, G, h, z, lam))
    s = h - np.einsum("bmn,bn->bm", G, z)
    stat = np.einsum("bij,bj->bi", P, z) + q + np.einsum("bmn,bm->bn", G, lam)
    return dict(dual=float(max(0.0, -lam.min())), primal=float(max(0.0, -s.min())),
                stationarity=float(np.abs(stat).max()), complementarity=float(np.abs(lam * s).max()))
