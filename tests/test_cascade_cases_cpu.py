"""The oracle alone on tests/_cascade_cases.py: what test_gpu_cascade.py leans
on, checked without a GPU so that no GPU test ever has to exclude a lane.

  * oracle.qp_exact solves every row of every case (status 0);
  * the cases reach what the golden fixtures never do: two and three hazard
    rows active at once, the box active alone, a large slack, wave counts
    0, 1, 2, 3 and K, and each of the four cars rows active;
  * the numpy ports of the closed forms (tests/_solver_ports.py, exact
    division) agree with the oracle to 1e-10 on all of it, slack included
    (measured: at most 2.6e-11).

Measured with this recipe, of 684 rows per K:
    K   hazard rows active 0 / 1 / 2 / 3   box only   |eps| > 0.1   wave counts
    1          228 / 456 /   0 /  0            35          171      0 1
    2          201 / 476 /   7 /  0            29          165      0 1 2
    3          188 / 379 / 115 /  2            28          262      0 1 3
    4          163 / 337 / 174 / 10            30          324      0 1 3 4
    5          171 / 250 / 252 / 11            21          318      0 1 3 4 5
    6          166 / 205 / 299 / 14            21          368      0 1 3 6
    7          161 / 195 / 306 / 22            23          351      0 2 3 5 6 7
    8          162 / 179 / 324 / 19            25          361      0 2 3 6 7 8
cars, of 300 rows: rows active on 129 / 17 / 6 / 21 lanes.
"""
import numpy as np
import pytest

import _cascade_cases as C
from _solver_ports import cars_qp_1d, uni_qp_2d


def test_batch_layout():
    """B ends neither on a wave nor on a workgroup; the second 320 rows are the
    first 320 with the kinds mixed into every wave."""
    assert C.UNI_B % 64 and C.UNI_B % 256 and C.UNI_B > 2 * 256
    assert C.CARS_B % 64 and C.CARS_B > 256
    d = C.unicycle(5)
    n = len(C.KINDS) * C.WAVE
    assert all((d["kind"][k * 64:(k + 1) * 64] == k).all() for k in range(len(C.KINDS)))
    for w in range(n // 64):
        assert len(np.unique(d["kind"][n + w * 64:n + (w + 1) * 64])) == len(C.KINDS)
    assert np.array_equal(np.sort(d["x"][:n], axis=0), np.sort(d["x"][n:2 * n], axis=0))
    assert (np.abs(d["u"]).max(1) > 2.5).sum() > 10  # rows whose u_nom alone leaves the box


@pytest.mark.parametrize("K", C.KS)
def test_oracle_solves_every_unicycle_row(K):
    r = C.reference(K)
    assert r["z"].shape == (C.UNI_B, 3)
    assert (r["status"] == 0).all() and np.isfinite(r["z"]).all()


def test_oracle_solves_every_cars_row():
    r = C.reference("cars")
    assert r["z"].shape == (C.CARS_B, 2)
    assert (r["status"] == 0).all() and np.isfinite(r["z"]).all()


@pytest.mark.parametrize("K", C.KS)
def test_unicycle_coverage(K):
    r = C.reference(K)
    n_act = r["act"][:, :K].sum(1)
    if K >= 3:
        assert (n_act == 2).mean() >= 0.10, np.bincount(n_act)
    if K >= 4:
        assert (n_act == 3).sum() >= 1, np.bincount(n_act)
    assert (r["act"][:, K:].any(1) & (n_act == 0)).sum() > 0   # the box alone
    assert (np.abs(r["z"][:, 2]) > 0.1).sum() > 100            # a slack the layer warns about


def test_wave_counts_over_the_sweep():
    """The live-row count the wave solves with (the port's, per 64 lanes): each
    of 0, 1, 2 and 3, and K itself for some K >= 4; and every slot solve that
    exists for a K (1, 2, 3 and K slots) is taken by some K."""
    seen, full = set(), set()
    for K in C.KS:
        r = C.reference(K)
        w = uni_qp_2d(r["Gn"], r["hn"], C.UNI_P, K)[2][::64]
        seen |= set(int(v) for v in w)
        if K >= 4 and (w == K).any():
            full.add(K)
    assert {0, 1, 2, 3} <= seen, seen
    assert full, "no K >= 4 whose wave solves with all K rows"


def test_cars_coverage():
    act = C.reference("cars")["act"]
    assert (act.sum(0) > 0).all(), act.sum(0)


@pytest.mark.parametrize("K", C.KS)
def test_port_matches_oracle_unicycle(K):
    r = C.reference(K)
    z2, _, _ = uni_qp_2d(r["Gn"], r["hn"], C.UNI_P, K)
    z3, _, _ = uni_qp_2d(r["Gn"], r["hn"], C.UNI_P, K, prune=False)
    assert C.rel(z2, r["z"]) <= 1e-10 and C.rel(z3, r["z"]) <= 1e-10


def test_port_matches_oracle_cars():
    r = C.reference("cars")
    assert C.rel(cars_qp_1d(r["Gn"], r["hn"], C.CARS_P), r["z"]) <= 1e-10
