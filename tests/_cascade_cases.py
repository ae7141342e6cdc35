"""Inputs for the Cascade layer's tests (CascadeCBFLayer.get_u_safe, the fp64
instantiation of cars_qp_1d / uni_qp_2d with P = diag(10, 1e-4, 1e7)),
importable without a GPU, and their reference: the oracle's rows
(oracle.{unicycle,cars}_build_cascade), oracle.normalize_rows, then
oracle.qp_exact on the diagonal P at its default tolerance.

The golden fixtures never have two hazard rows active at once; these states
are placed so that they do.

Unicycle, K = 1..8 hazards on a ring of radius 0.95 (neighbours bind
together), five kinds of state of 64 lanes each:
  far       radius U[4, 6] from the origin (no hazard row can bind)
  rim       a hazard centre + U[0.6, 0.8] in a random direction
  ring      x, y ~ U[-0.5, 0.5], inside the ring of hazards
  inside    a hazard centre + N(0, 0.05)
  outer     a hazard centre + U[0.7, 0.9] along the hazard's own outward
            direction, +-0.3 rad
Batch: one wave per kind (320 rows), the same rows interleaved lane by lane
so that every wave mixes the kinds (320), then 44 fresh rows: B = 684 ends
neither on a wave nor on a workgroup, and the first 256 rows (what the
one-workgroup path takes) are the far, rim, ring and inside waves.

Cars: the base state + N(0, 1) with car 3 pulled to within U[3.3, 4.5] of
car 2, car 4 to within U[3.3, 4.5] of car 3, or both to U[3.4, 3.8]
(100 rows each, B = 300), v3 += N(0, 3), u_nom ~ U[-12, 12].
"""
import functools

import numpy as np

from oracle import oracle as O

GAMMA_B, K_D, L_P = 40.0, 3.0, 0.03   # unicycle layer arguments
CARS_GAMMA_B = 20.0
KS = tuple(range(1, 9))
KINDS = ("far", "rim", "ring", "inside", "outer")
WAVE = 64
TAIL = 44
UNI_B = 2 * len(KINDS) * WAVE + TAIL
CARS_B = 300
UNI_P = np.array([10.0, 1e-4, 1e7])
CARS_P = np.array([0.1, 10.0])
CARS_BASE = np.array([34.0, 30.0, 28.0, 30.0, 22.0, 30.0, 16.0, 35.0, 10.0, 30.0])


def hazards(K):
    a = 2.0 * np.pi * np.arange(K) / K
    return 0.95 * np.stack([np.cos(a), np.sin(a)], 1)


def _uni_xy(rng, kind, n, hz):
    K = len(hz)
    j = rng.integers(0, K, n)
    if kind == "far":
        r, a = rng.uniform(4.0, 6.0, n), rng.uniform(-np.pi, np.pi, n)
        return np.stack([r * np.cos(a), r * np.sin(a)], 1)
    if kind == "rim":
        r, a = rng.uniform(0.6, 0.8, n), rng.uniform(-np.pi, np.pi, n)
        return hz[j] + np.stack([r * np.cos(a), r * np.sin(a)], 1)
    if kind == "ring":
        return rng.uniform(-0.5, 0.5, (n, 2))
    if kind == "inside":
        return hz[j] + rng.normal(0.0, 0.05, (n, 2))
    r = rng.uniform(0.7, 0.9, n)
    a = 2.0 * np.pi * j / K + rng.uniform(-0.3, 0.3, n)
    return hz[j] + np.stack([r * np.cos(a), r * np.sin(a)], 1)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def unicycle(K):
    """dict(hazards, x (B,3), u (B,2), mu (B,3), sigma (B,3), kind (B,) index into KINDS); read-only."""
    rng = np.random.default_rng(1000 + K)
    hz = hazards(K)
    xy = np.concatenate([_uni_xy(rng, kind, WAVE, hz) for kind in KINDS])
    kind = np.repeat(np.arange(len(KINDS)), WAVE)
    x = np.concatenate([xy, rng.uniform(-np.pi, np.pi, (len(xy), 1))], 1)
    u = rng.uniform(-1.0, 1.0, (len(x), 2))
    mu = rng.normal(0.0, 0.1, (len(x), 3))
    sigma = rng.uniform(0.0, 0.3, (len(x), 3))
    n = len(x)
    mix = (np.arange(n) % len(KINDS)) * WAVE + np.arange(n) // len(KINDS)  # lane by lane through the kinds
    tk = np.arange(TAIL) % len(KINDS)
    txy = np.concatenate([_uni_xy(rng, KINDS[k], 1, hz) for k in tk])
    tx = np.concatenate([txy, rng.uniform(-np.pi, np.pi, (TAIL, 1))], 1)
    x = np.concatenate([x, x[mix], tx])
    u = np.concatenate([u, u[mix], rng.uniform(-1.0, 1.0, (TAIL, 2))])
    mu = np.concatenate([mu, mu[mix], rng.normal(0.0, 0.1, (TAIL, 3))])
    sigma = np.concatenate([sigma, sigma[mix], rng.uniform(0.0, 0.3, (TAIL, 3))])
    kind = np.concatenate([kind, kind[mix], tk])
    u[::5] *= 3.0  # the +-2.5 box binds on its own
    assert len(x) == UNI_B
    return _freeze(dict(hazards=hz, x=x, u=u, mu=mu, sigma=sigma, kind=kind))


@functools.lru_cache(maxsize=None)
def cars():
    """dict(x (B,10), u (B,1), mu, sigma (B,10): what the cars layer ignores); read-only."""
    rng = np.random.default_rng(2000)
    B, n = CARS_B, CARS_B // 3
    x = CARS_BASE + rng.normal(0.0, 1.0, (B, 10))
    g0, g1, g2 = slice(0, n), slice(n, 2 * n), slice(2 * n, B)
    x[g0, 6] = x[g0, 4] - rng.uniform(3.3, 4.5, n)
    x[g1, 8] = x[g1, 6] - rng.uniform(3.3, 4.5, n)
    x[g2, 6] = x[g2, 4] - rng.uniform(3.4, 3.8, B - 2 * n)
    x[g2, 8] = x[g2, 6] - rng.uniform(3.4, 3.8, B - 2 * n)
    x[:, 7] += rng.normal(0.0, 3.0, B)
    u = rng.uniform(-12.0, 12.0, (B, 1))
    mu = rng.normal(0.0, 0.1, (B, 10))
    sigma = np.tile(np.array(O.MAX_STD["SimulatedCars"]), (B, 1)) * rng.uniform(0.0, 1.5, (B, 1))
    return _freeze(dict(x=x, u=u, mu=mu, sigma=sigma))


def case(name):
    """`name` is 'cars' or a hazard count 1..8."""
    return cars() if name == "cars" else unicycle(int(name))


def pdiag(name):
    return CARS_P if name == "cars" else UNI_P


def rows(name, d=None):
    """The oracle's raw rows (G, h) of a case (or of inputs `d` laid out like it)."""
    d = case(name) if d is None else d
    if name == "cars":
        _, G, h = O.cars_build_cascade(d["x"], d["u"], CARS_GAMMA_B)
    else:
        _, G, h = O.unicycle_build_cascade(d["x"], d["u"], d["mu"], d["sigma"], GAMMA_B, K_D, hazards(int(name)))
    return G, h


def solve(name, d=None):
    """dict(G, h, Gn, hn, z, act, status): rows, normalised rows and oracle.qp_exact on them."""
    G, h = rows(name, d)
    Gn, hn, _ = O.normalize_rows(G, h)
    z, _, act, st = O.qp_exact(pdiag(name), Gn, hn)
    return dict(G=G, h=h, Gn=Gn, hn=hn, z=z, act=act, status=st)


@functools.lru_cache(maxsize=None)
def reference(name):
    """solve(name) on the case itself, computed once and read-only."""
    return _freeze(solve(name))


def rel(a, b):
    """max |a - b| / max(1, |b|); inf if a holds a NaN where b does not."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return float(np.max(np.where(np.isnan(e), np.inf, e))) if a.size else 0.0
