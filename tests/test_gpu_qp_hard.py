"""The generic QP kernels (rcbf_qp_solve, rcbf_qp_solve_f64, rcbf_qp_solve_saved,
rcbf_qp_backward, rcbf_qp_backward_saved) on the problems random Gaussian QPs
never produce, through the C-ABI so that the per-lane status is visible.

Shapes: every n in {1, 2, 3} with m in {1, 4, 5, 8, 9, 12, 13, 16} (both sides
of each row-padding bucket, the fp64 m > 12 launches that need more than
64 KiB of LDS) and (3, 7) (exact-size kernels in fp32, padded in fp64);
B = 300 = 128 + 128 + 44 lanes, and B in {1, 127, 129}.

Cases: tests/_qp_cases.py -- QPs built backwards from their KKT point, so the
optimum z* is known without a solver: duplicate, parallel and antiparallel
rows, more than n tight rows, tight rows with a zero multiplier, infeasible
pairs, near-degenerate and ill-conditioned fp64 data -- and random_qps.

Checkers: z* itself (normalize = 0); oracle.qp_exact_general on
oracle.normalize_rows(G, h) in the entry point's dtype (normalize = 1), which
must report status 0 on every QP.  No lane is excluded anywhere, except by the
existing _non_degenerate rule of the backward tests.

Bars, all relative to max(1, |z|), from the project's existing tests:
fp32 z 1e-6 (exact solvers) / 1e-5 (PDIPM); fp64 z 1e-9, 1e-7 on 'near' and
'illcond' (the Cascade unicycle bar); multipliers of the fp32 entry point as
test_large_batch_properties (primal 1e-5, stationarity 1e-4 (1 + max lam),
complementarity 1e-4).

Multipliers of the fp64 entry point (test_fp64_multipliers): per family,
100 x the oracle's own worst KKT residual on the same inputs, floor 1e-12.
ORACLE_KKT64 below holds the oracle's residuals, measured on the CPU on
cases() over every shape, raw and fp64-normalised rows.  ('near' primal
3.1e-9: the oracle accepts a candidate that violates a row by tol * scale,
which slacks and multipliers down to 1e-11 and 1e-9 reach.)

rcbf_qp_solve_saved's fp64 solution is held to the fp64 bar on every family.
With normalize = 1 the reference for 'weak' and 'vertex' is the oracle at
tol = 1e-13: the fp32 quotients move their tight rows by ~1e-8, and at its
default tol = 1e-10 the oracle accepts a row violated by tol * scale ~ 5e-9
and returns a neighbouring vertex 3e-8 away.  At 1e-13 it solves every QP
(status 0 asserted) and agrees with tol = 1e-14 exactly.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _qp_cases as C
from oracle import oracle as O
from test_gpu_qp_backward import _layer, _non_degenerate
from test_qp_backward_cpu import random_qps

pytestmark = pytest.mark.gpu

B = 300
F32, F64 = "f32", "f64"
_TD = {F32: torch.float32, F64: torch.float64}
_ND = {F32: np.float32, F64: np.float64}
SOLVERS = (0, 1, 2)
OK, MAX_ITER, INFEASIBLE, NONFINITE = 0, 1, 2, 3

# the oracle's own KKT residuals per family (module docstring): dual, primal, stationarity, complementarity
ORACLE_KKT64 = {
    "full": (0, 4.5e-15, 1.5e-14, 2.0e-14), "diag": (0, 5.4e-15, 5.4e-15, 2.5e-14),
    "weak": (0, 4.7e-14, 2.5e-14, 2.7e-13), "vertex": (0, 1.5e-13, 1.1e-14, 2.4e-13),
    "dup": (0, 3.6e-15, 1.5e-14, 1.6e-14), "parallel": (0, 5.4e-15, 1.1e-14, 1.7e-14),
    "antiparallel_feasible": (0, 5.4e-15, 1.5e-14, 1.7e-14), "near": (0, 3.1e-9, 1.1e-14, 3.5e-19),
    "illcond": (0, 1.0e-15, 8.9e-16, 1.9e-15), "gauss": (0, 9.5e-16, 3.6e-15, 9.0e-15)}


def kkt64_bars(fam):
    """100 x the oracle's residuals on this family, floor 1e-12."""
    return {k: max(100.0 * v, 1e-12)
            for k, v in zip(("dual", "primal", "stationarity", "complementarity"), ORACLE_KKT64[fam])}


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return float(np.max(np.where(np.isnan(e), np.inf, e))) if a.size else 0.0


def z_bar(dtype, solver, fam):
    if dtype == F32:
        return 1e-5 if solver == 1 else 1e-6
    return 1e-7 if fam in C.FP64_ONLY else 1e-9


@functools.lru_cache(maxsize=None)
def _prm(solver):
    from rcbf_amd import _lib
    p = _lib.RcbfParams.from_buffer_copy(_layer()._prm)
    p.solver = solver
    return p


def families(dtype):
    return C.DYADIC + (C.FP64_ONLY if dtype == F64 else ()) + ("gauss",)


@functools.lru_cache(maxsize=None)
def cases(n, m):
    """Every family at B lanes for one shape (fp64 arrays; read-only)."""
    rng = np.random.default_rng(977 * n + m)
    out = {fam: C.kkt_qps(rng, B, n, m, fam) for fam in C.FEASIBLE}
    P, q, G, h = random_qps(rng, B, n, m)
    out["gauss"] = dict(P=P, q=q.astype(np.float64), G=G.astype(np.float64), h=h.astype(np.float64))
    if m >= 2:
        out["infeasible"] = C.kkt_qps(rng, B, n, m, "infeasible")
    for d in out.values():
        for a in d.values():
            a.setflags(write=False)
    return out


def normalized(d, dtype):
    """The rows the kernel solves with normalize = 1, as fp64 values."""
    Gn, hn, _ = O.normalize_rows(d["G"].astype(_ND[dtype]), d["h"].astype(_ND[dtype]))
    return Gn.astype(np.float64), hn.astype(np.float64)


@functools.lru_cache(maxsize=None)
def refs(n, m, dtype):
    """The oracle's optimum on the normalised rows of every family of
    families(dtype), in one call; it must solve every QP."""
    cs = cases(n, m)
    fams = families(dtype)
    Gn, hn = zip(*(normalized(cs[f], dtype) for f in fams))
    z, _, _, st = O.qp_exact_general(np.concatenate([cs[f]["P"] for f in fams]),
                                     np.concatenate([cs[f]["q"] for f in fams]), np.concatenate(Gn), np.concatenate(hn))
    out = {}
    for i, f in enumerate(fams):
        assert (st[i * B:(i + 1) * B] == 0).all(), ("the oracle left a QP unsolved", n, m, dtype, f)
        out[f] = z[i * B:(i + 1) * B]
    return out


@functools.lru_cache(maxsize=None)
def refs_tight(n, m):
    """'weak' and 'vertex' on their fp32-normalised rows with the oracle at
    tol = 1e-13 (module docstring): the reference of the fp64 bar there."""
    cs = cases(n, m)
    out = {}
    for f in ("weak", "vertex"):
        Gn, hn = normalized(cs[f], F32)
        z, _, _, st = O.qp_exact_general(cs[f]["P"], cs[f]["q"], Gn, hn, tol=1e-13)
        assert (st == 0).all(), ("the oracle left a QP unsolved", n, m, f)
        out[f] = z
    return out


def _offset_view(t):
    """t's values in a view that starts one element into a larger buffer
    (sentinels before and after)."""
    buf = torch.full((t.numel() + 2,), 12345, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def solve(solver, d, normalize, dtype, lam=False, status=True, flag=0, saved=False, offset=False, nb=None):
    """One launch of rcbf_qp_solve / _f64 / _saved on the QPs d (the first nb
    of them).  Returns dict(z, lam, st, flag, z64 [, guards])."""
    from rcbf_amd import _lib
    lib = _lib.load()
    td = _TD[dtype]
    nb = d["G"].shape[0] if nb is None else nb
    _, m, n = d["G"].shape
    bufs = []

    def place(t):
        if not offset:
            return t
        buf, v = _offset_view(t)
        bufs.append(buf)
        return v

    ins = [place(torch.as_tensor(np.array(d[k][:nb]), dtype=td, device="cuda")) for k in "PqGh"]
    z = place(torch.full((nb, n), float("nan"), dtype=td, device="cuda"))
    second = None
    if saved:
        second = place(torch.full((nb, n), float("nan"), dtype=torch.float64, device="cuda"))
    elif lam:
        second = place(torch.full((nb, m), float("nan"), dtype=torch.float64, device="cuda"))
    st = place(torch.full((nb,), -1, dtype=torch.int32, device="cuda")) if status else None
    fl = torch.tensor([flag], dtype=torch.int32, device="cuda") if flag is not None else None
    fn = lib.rcbf_qp_solve_saved if saved else (lib.rcbf_qp_solve_f64 if dtype == F64 else lib.rcbf_qp_solve)
    rc = fn(ctypes.byref(_prm(solver)), nb, n, m, *[_lib.ptr(t) for t in ins], normalize, _lib.ptr(z),
            _lib.ptr(second), _lib.ptr(st), _lib.ptr(fl), _lib.stream_of(z.device))
    assert rc == 0
    torch.cuda.synchronize()
    out = dict(z=z.cpu().numpy(), st=None if st is None else st.cpu().numpy(),
               flag=None if fl is None else int(fl.item()))
    out["z64" if saved else "lam"] = None if second is None else second.cpu().numpy()
    if offset:
        out["guards"] = all(float(b[0]) == 12345 and float(b[-1]) == 12345 for b in bufs)
    return out


def kkt_errors(d, Gk, hk, z, lam, dtype, fam, tag):
    """KKT of (z, lam) on the rows the kernel solved; a list of complaints."""
    r = C.kkt_residuals(d["P"], d["q"], Gk, hk, z, lam)
    if dtype == F32:
        bars = dict(dual=0.0, primal=1e-5, stationarity=1e-4 * (1 + np.abs(lam).max()), complementarity=1e-4)
    else:
        bars = kkt64_bars(fam)
    bad = [f"{tag}: {k} residual {r[k]:.3g} > {bars[k]:.3g}" for k in r if not r[k] <= bars[k]]
    if not np.isfinite(lam).all():
        bad.append(f"{tag}: non-finite multipliers")
    return bad


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,m", C.SHAPES)
def test_forward_status_and_multipliers(n, m, dtype):
    """z_out, status_out, fail_flag and lam_out of rcbf_qp_solve[_f64] (all
    three solvers), and rcbf_qp_solve_saved's fp64 solution, on every family."""
    cs, ref = cases(n, m), refs(n, m, dtype)
    errs = []
    for fam in families(dtype):
        d = cs[fam]
        for normalize in (0, 1):
            if normalize == 0 and fam == "gauss":
                continue  # no constructed optimum
            want = ref[fam] if normalize else d["z"]
            Gk, hk = normalized(d, dtype) if normalize else (d["G"], d["h"])
            for solver in SOLVERS:
                tag = f"{fam} normalize={normalize} solver={solver}"
                bar = z_bar(dtype, solver, fam)
                for with_lam in (False, True):
                    o = solve(solver, d, normalize, dtype, lam=with_lam)
                    e = rel(o["z"], want)
                    if not e <= bar:
                        errs.append(f"{tag} lam_out={with_lam}: z off by {e:.3g} > {bar:.3g} "
                                    f"(lane {int(np.argmax(np.abs(o['z'] - want).max(axis=1)))})")
                    if (o["st"] != OK).any() or o["flag"] != 0:
                        errs.append(f"{tag} lam_out={with_lam}: status {np.unique(o['st'])} flag {o['flag']:#x}")
                    if with_lam and dtype == F32:  # the fp64 entry point's: test_fp64_multipliers
                        errs += kkt_errors(d, Gk, hk, o["z"].astype(np.float64), o["lam"], dtype, fam, tag)
                if dtype == F32:
                    o = solve(solver, d, normalize, F32, saved=True)
                    if not np.array_equal(o["z64"].astype(np.float32).view(np.uint32), o["z"].view(np.uint32)):
                        errs.append(f"{tag}: float(z64_saved) != z_out")
                    tight = normalize and fam in ("weak", "vertex")
                    e = rel(o["z64"], refs_tight(n, m)[fam] if tight else want)
                    if not e <= z_bar(F64, solver, fam):
                        errs.append(f"{tag}: z64_saved off by {e:.3g}")
                    if (o["st"] != OK).any() or o["flag"] != 0:
                        errs.append(f"{tag} saved: status {np.unique(o['st'])} flag {o['flag']:#x}")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("n,m", C.SHAPES)
def test_fp64_multipliers(n, m):
    """KKT of rcbf_qp_solve_f64's lam_out on the rows the kernel solved, every
    family, all three solvers: each family at 100 x the oracle's own residuals
    on it, floor 1e-12 (kkt64_bars).

    'illcond' (P = diag(1, 1e-2, 1e5) or diag(10, 1e-4, 1e7)) has a tight row
    whose multiplier is 0.  Before gi_solve dropped rows with a negative
    recomputed multiplier, Goldfarb-Idnani ended on the vertex that holds it
    and the polish recomputed the multipliers there as -G_A^-T (P z + q):
    z_3 ~ 1e-7 carries the vertex solve's absolute error ~1e-16, P_33 = 1e7
    turns it into 1e-9, and the zero multiplier came out as -5e-10
    (stationarity of lam_out up to 3.3e-9 at n = 3)."""
    cs = cases(n, m)
    errs = []
    for fam in families(F64):
        d = cs[fam]
        for normalize in (0, 1):
            Gk, hk = normalized(d, F64) if normalize else (d["G"], d["h"])
            for solver in SOLVERS:
                o = solve(solver, d, normalize, F64, lam=True)
                errs += kkt_errors(d, Gk, hk, o["z"], o["lam"], F64, fam, f"{fam} normalize={normalize} solver={solver}")
    assert not errs, "\n".join(errs)


def test_pdipm_thin_slab_by_value():
    """Two QPs of 'near' whose rows hold both sides of a slab 1e-9 wide.  The
    interior point's polish picked the two (dependent) sides as its active
    set; the singular vertex solve ran z off along the slab (-1.2e5 and 4e9)
    with multipliers +inf, and the KKT certificate, which tested feasibility
    and the multipliers' sign but not stationarity, passed it with status 0."""
    d = dict(P=np.array([[[7.0, 1.0], [1.0, 4.0]], [[10.0, -6.0], [-6.0, 7.0]]]),
             q=np.array([[7.499998, -3.749999], [-7.999998, 10.750001]]),
             G=np.array([[[0.4, -0.4], [0.400199900049975, -0.399800099950025], [0.8, 0.0],
                          [-0.3999999999984, 0.3999999999984]],
                         [[-1.0, 0.001], [-0.5, -0.5], [0.50000000025, 0.50000000025], [-1.0, 0.0]]]),
             h=np.array([[-1.0, -1.0, -1.0, 1.0], [0.24825, 1.0, -1.0, 0.25]]))
    z_star = np.array([[-1.25, 1.25], [-0.25, -1.75]])
    for solver in SOLVERS:
        o = solve(solver, d, 0, F64, lam=True)
        assert (o["st"] == OK).all() and o["flag"] == 0, solver
        assert rel(o["z"], z_star) <= 1e-7, (solver, o["z"])
        assert not kkt_errors(d, d["G"], d["h"], o["z"], o["lam"], F64, "near", f"solver={solver}")


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("nb", [1, 127, 129])
@pytest.mark.parametrize("n,m", [(1, 5), (2, 8), (3, 13)])
def test_small_and_ragged_batches(n, m, nb, dtype):
    """One lane, a block one lane short and one lane over: predicated staging,
    and the lanes past the batch leave before the wave's ballots."""
    cs, ref = cases(n, m), refs(n, m, dtype)
    errs = []
    for fam in ("full", "diag", "vertex", "gauss"):
        d = cs[fam]
        for normalize in (0, 1):
            if normalize == 0 and fam == "gauss":
                continue
            want = (ref[fam] if normalize else d["z"])[:nb]
            for solver in SOLVERS:
                o = solve(solver, d, normalize, dtype, nb=nb)
                e = rel(o["z"], want)
                if not e <= z_bar(dtype, solver, fam) or (o["st"] != OK).any() or o["flag"] != 0:
                    errs.append(f"{fam} normalize={normalize} solver={solver}: z off by {e:.3g}, "
                                f"status {np.unique(o['st'])}, flag {o['flag']:#x}")
    assert not errs, "\n".join(errs)


def _with_infeasible(cs):
    """'full' with every fourth lane taken from 'infeasible': both kinds in every wave."""
    bad = np.arange(B) % 4 == 3
    d = {k: np.where(bad.reshape((B,) + (1,) * (cs["full"][k].ndim - 1)), cs["infeasible"][k], cs["full"][k])
         for k in ("P", "q", "G", "h", "z")}
    return d, bad


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n,m", [(1, 4), (2, 5), (3, 7), (3, 16)])
def test_failure_reporting(n, m, dtype, capsys):
    """Infeasible lanes among feasible ones: the per-lane status, the OR-ed
    fail_flag bits, and the neighbours' solutions."""
    d, bad = _with_infeasible(cases(n, m))
    errs = []
    for solver in SOLVERS:
        for normalize in (0, 1):
            tag = f"solver={solver} normalize={normalize}"
            want = (refs(n, m, dtype)["full"] if normalize else d["z"])[~bad]
            o = solve(solver, d, normalize, dtype, flag=1 << 30)
            st = o["st"]
            if (st[~bad] != OK).any():
                errs.append(f"{tag}: a feasible lane reports {np.unique(st[~bad])}")
            e = rel(o["z"][~bad], want)
            if not e <= z_bar(dtype, solver, "full"):
                errs.append(f"{tag}: feasible lanes off by {e:.3g}")
            if solver == 1:
                with capsys.disabled():
                    print(f"\n  PDIPM ({n},{m},{dtype}) {tag}: infeasible lanes report {np.unique(st[bad])}")
                if (st[bad] == OK).any() or (st[bad] < 0).any() or (st[bad] > NONFINITE).any():
                    errs.append(f"{tag}: PDIPM calls an infeasible lane {np.unique(st[bad])}")
            elif (st[bad] != INFEASIBLE).any():
                errs.append(f"{tag}: infeasible lanes report {np.unique(st[bad])}")
            expect = 1 << 30
            for s in st[st != OK]:
                expect |= 1 << int(s)
            if o["flag"] != expect:
                errs.append(f"{tag}: fail_flag {o['flag']:#x}, expected {expect:#x}")
            # each reporting output works without the other
            o1 = solve(solver, d, normalize, dtype, status=False, flag=0)
            o2 = solve(solver, d, normalize, dtype, status=True, flag=None)
            if o1["flag"] != expect & ~(1 << 30) or not np.array_equal(o2["st"], st):
                errs.append(f"{tag}: status_out / fail_flag alone: {o1['flag']:#x}, {np.unique(o2['st'])}")
            for oo in (o1, o2):
                if not np.array_equal(oo["z"][~bad], o["z"][~bad]):
                    errs.append(f"{tag}: z changes with the reporting outputs")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_all_zero_row(dtype):
    """A row [0 | h] among the QP's rows: with normalize = 1 and h = 0 its
    0 / 0 is RCBF_QP_NONFINITE on that lane only; without normalisation
    0 z <= 1 changes nothing and 0 z <= -1 is RCBF_QP_INFEASIBLE (solvers 0
    and 2; for the interior point any status but OK is accepted, the leniency
    it has on every infeasible lane in test_failure_reporting)."""
    n, m = 2, 5
    cs = cases(n, m)
    src = cs["full"]
    slack = src["h"] - np.einsum("bmn,bn->bm", src["G"], src["z"])
    loose = np.argmax(slack > 0, axis=1)               # a row that is not tight: z* does not depend on it
    assert (slack[np.arange(B), loose] > 0).all()
    hit = np.zeros(B, bool); hit[[3, 70, 130, 191, 299]] = True

    def edit(rows, hval):
        d = {k: src[k].copy() for k in ("P", "q", "G", "h", "z")}
        d["G"][rows, loose[rows]] = 0.0
        d["h"][rows, loose[rows]] = hval
        return d

    errs = []
    for solver in SOLVERS:
        clean = solve(solver, src, 1, dtype)
        o = solve(solver, edit(hit, 0.0), 1, dtype, flag=0)
        if (o["st"][hit] != NONFINITE).any() or (o["st"][~hit] != OK).any() or o["flag"] != 1 << NONFINITE:
            errs.append(f"solver={solver} [0|0] normalised: status {o['st'][hit]}, others "
                        f"{np.unique(o['st'][~hit])}, flag {o['flag']:#x}")
        if not np.array_equal(o["z"][~hit], clean["z"][~hit]):
            errs.append(f"solver={solver} [0|0] normalised: a neighbour's z changed")
        o = solve(solver, edit(np.ones(B, bool), 1.0), 0, dtype, flag=0)
        e = rel(o["z"], src["z"])
        if not e <= z_bar(dtype, solver, "full") or (o["st"] != OK).any() or o["flag"] != 0:
            errs.append(f"solver={solver} [0|1]: z off by {e:.3g}, status {np.unique(o['st'])}")
        o = solve(solver, edit(hit, -1.0), 0, dtype, flag=0)
        e = rel(o["z"][~hit], src["z"][~hit])
        bad_st = o["st"][hit]
        wrong = (bad_st == OK).any() if solver == 1 else (bad_st != INFEASIBLE).any()
        if wrong or (o["st"][~hit] != OK).any() or not e <= z_bar(dtype, solver, "full"):
            errs.append(f"solver={solver} [0|-1]: status {bad_st}, others {np.unique(o['st'][~hit])}, off {e:.3g}")
    assert not errs, "\n".join(errs)


def test_solve_qp_raises_on_one_infeasible_lane():
    """CBFQPLayer.solve_qp: one infeasible lane in the batch raises the
    reference's exception; the next clean batch solves."""
    n, m = 3, 7
    cs = cases(n, m)
    d = {k: cs["full"][k].copy() for k in ("P", "q", "G", "h")}
    for k in d:
        d[k][200] = cs["infeasible"][k][200]
    layer = _layer()
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")
    with pytest.raises(Exception, match="QP Failed to solve"):
        layer.solve_qp(*(dev(d[k]) for k in "PqGh"))
    z = layer.solve_qp(*(dev(cs["full"][k]) for k in "PqGh"))
    assert rel(z.cpu().numpy(), refs(n, m, F32)["full"][:, :-1]) <= 1e-6


def _mixed(golden, fixture, kind):
    """B layer rows of a golden fixture and a copy with one lane per wave, at
    a different position in each, replaced by a QP that breaks the layer
    structure.  Returns (layer-only dict, mixed dict, touched mask)."""
    g = golden(fixture)
    base = {k: g["rand_" + k][:B].astype(np.float32).astype(np.float64) for k in ("P", "q", "G", "h")}
    _, m, n = base["G"].shape
    mix = {k: v.copy() for k, v in base.items()}
    lanes = np.array([w * 64 + (5 + 13 * w) % (64 if w < 4 else B - 256) for w in range(5)])
    full = cases(n, m)["full"]
    for i in lanes:
        if kind == "dense":
            for k in mix:
                mix[k][i] = full[k][i]
        elif kind == "q":
            mix["q"][i] = np.array([0.5, -0.25, 0.125][:n])
        else:
            mix["G"][i, m - 1, n - 1] = 0.5     # the last actuator row reaches into the slack column
    touched = np.zeros(B, bool); touched[lanes] = True
    return base, mix, touched


@pytest.mark.parametrize("kind", ["dense", "q", "row"])
@pytest.mark.parametrize("fixture", ["cars_layer", "unicycle3_layer"])
def test_mixed_waves_forward(golden, fixture, kind):
    """One lane per wave breaks the layer structure (a dense P, a non-zero q,
    a non-layer row): the wave's ballot sends it to the general solver, and
    every lane still has its own optimum.  The untouched lanes are compared
    with the all-layer launch (closed form against Goldfarb-Idnani) on the
    fp64 solution rcbf_qp_solve_saved returns: 1e-9 absolute is below the
    fp32 output's own resolution."""
    base, mix, touched = _mixed(golden, fixture, kind)
    Gn, hn = normalized(mix, F32)
    want, _, _, st = O.qp_exact_general(mix["P"], mix["q"], Gn, hn)
    assert (st == 0).all()
    errs = []
    for solver in SOLVERS:
        o = solve(solver, mix, 1, F32)
        e = rel(o["z"], want)
        if not e <= z_bar(F32, solver, "") or (o["st"] != OK).any() or o["flag"] != 0:
            errs.append(f"solver={solver}: z off by {e:.3g}, status {np.unique(o['st'])}")
        a, b = solve(solver, base, 1, F32, saved=True), solve(solver, mix, 1, F32, saved=True)
        gap = float(np.abs(a["z64"][~touched] - b["z64"][~touched]).max())
        if not gap <= 1e-9:
            errs.append(f"solver={solver}: untouched lanes moved by {gap:.3g}")
        if not np.array_equal(b["z"], o["z"]):
            errs.append(f"solver={solver}: rcbf_qp_solve_saved's z differs from rcbf_qp_solve's")
    assert not errs, "\n".join(errs)


def backward(d, w, normalize, saved=False, offset=False, solver=0):
    """rcbf_qp_backward, or the saved pair, on the QPs d: the four gradients."""
    from rcbf_amd import _lib
    lib = _lib.load()
    nb, m, n = d["G"].shape
    bufs = []

    def place(t):
        if not offset:
            return t
        buf, v = _offset_view(t)
        bufs.append(buf)
        return v

    f32 = lambda a: torch.as_tensor(np.array(a), dtype=torch.float32, device="cuda")
    ins = [place(f32(d[k])) for k in "PqGh"]
    wd = place(f32(w))
    outs = [place(torch.full_like(t, float("nan"))) for t in ins]
    s = _lib.stream_of(wd.device)
    prm = ctypes.byref(_prm(solver))
    if saved:
        z = torch.empty(nb, n, device="cuda")
        z64 = torch.empty(nb, n, dtype=torch.float64, device="cuda")
        assert lib.rcbf_qp_solve_saved(prm, nb, n, m, *[_lib.ptr(t) for t in ins], normalize, _lib.ptr(z),
                                       _lib.ptr(z64), None, None, s) == 0
        assert lib.rcbf_qp_backward_saved(prm, nb, n, m, *[_lib.ptr(t) for t in ins], normalize, _lib.ptr(z64),
                                          _lib.ptr(wd), *[_lib.ptr(t) for t in outs], s) == 0
    else:
        assert lib.rcbf_qp_backward(prm, nb, n, m, *[_lib.ptr(t) for t in ins], normalize, _lib.ptr(wd),
                                    *[_lib.ptr(t) for t in outs], s) == 0
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in zip("PqGh", outs)}
    if offset:
        out["guards"] = all(float(b[0]) == 12345 and float(b[-1]) == 12345 for b in bufs)
    return out


@pytest.mark.parametrize("kind", ["dense", "q", "row"])
@pytest.mark.parametrize("fixture", ["cars_layer", "unicycle3_layer"])
def test_mixed_waves_backward(golden, fixture, kind):
    """rcbf_qp_backward on the same mixed waves: the oracle's gradients on
    every non-degenerate lane, and the all-layer launch's on the untouched
    ones."""
    base, mix, touched = _mixed(golden, fixture, kind)
    n = mix["q"].shape[1]
    w = np.random.default_rng(9).normal(0, 1, (B, n)).astype(np.float32)
    want = O.qp_backward(mix["P"], mix["q"], mix["G"], mix["h"], True, w)
    ok = _non_degenerate(mix["P"], mix["q"], mix["G"].astype(np.float32), mix["h"].astype(np.float32), 1)
    assert ok.mean() > 0.9
    got, ref = backward(mix, w, 1), backward(base, w, 1)
    errs = []
    for k in "PqGh":
        e = rel(got[k][ok], want[k][ok])
        if not e <= 1e-5:
            errs.append(f"grad_{k} off by {e:.3g}")
        sel = ok & ~touched
        gap = float(np.abs(got[k][sel].astype(np.float64) - ref[k][sel]).max())
        if not gap <= 1e-9:
            errs.append(f"grad_{k}: untouched lanes moved by {gap:.3g}")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("n,m", [(3, 5), (2, 4)])
def test_misaligned_base_pointers(n, m):
    """Every input and output one element into a larger buffer (m n odd and
    even): the scalar staging branch gives the aligned launch's bits and
    writes nothing outside its tensors."""
    cs = cases(n, m)
    errs = []
    for fam in ("full", "vertex"):
        d = cs[fam]
        for solver in SOLVERS:
            for normalize in (0, 1):
                for kw in (dict(lam=True), dict(saved=True)):
                    a = solve(solver, d, normalize, F32, **kw)
                    b = solve(solver, d, normalize, F32, offset=True, **kw)
                    for k in ("z", "lam", "z64", "st"):
                        if a.get(k) is not None and a[k].tobytes() != b[k].tobytes():
                            errs.append(f"{fam} solver={solver} normalize={normalize} {kw}: {k} differs")
                    if not b["guards"]:
                        errs.append(f"{fam} solver={solver} normalize={normalize} {kw}: a guard element was written")
        w = np.random.default_rng(3).normal(0, 1, (B, n)).astype(np.float32)
        for normalize in (0, 1):
            for saved in (False, True):
                a = backward(d, w, normalize, saved=saved)
                b = backward(d, w, normalize, saved=saved, offset=True)
                for k in "PqGh":
                    if a[k].tobytes() != b[k].tobytes():
                        errs.append(f"{fam} backward saved={saved} normalize={normalize}: grad_{k} differs")
                if not b["guards"]:
                    errs.append(f"{fam} backward saved={saved} normalize={normalize}: a guard element was written")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (2, 5), (2, 8), (2, 16), (3, 4), (3, 8), (3, 12), (3, 13), (3, 16)])
def test_backward_shape_sweep(n, m, normalize):
    """rcbf_qp_backward and the saved pair over the row-padding buckets and
    n = 1, with a partial last block: random QPs against oracle.qp_backward
    on the non-degenerate lanes (the existing rule); on 'weak', 'vertex' and
    'dup', where the derivative jumps, finite gradients everywhere and the
    oracle's grad_q where the lane is non-degenerate."""
    cs = cases(n, m)
    w = np.random.default_rng(13 * n + m).normal(0, 1, (B, n)).astype(np.float32)
    d = cs["gauss"]
    want = O.qp_backward(d["P"], d["q"], d["G"], d["h"], bool(normalize), w)
    ok = _non_degenerate(d["P"], d["q"], d["G"].astype(np.float32), d["h"].astype(np.float32), normalize)
    assert ok.mean() > 0.9
    errs = []
    for saved in (False, True):
        got = backward(d, w, normalize, saved=saved)
        for k in "PqGh":
            e = rel(got[k][ok], want[k][ok])
            if not e <= 1e-5:
                errs.append(f"gauss saved={saved}: grad_{k} off by {e:.3g}")
    for fam in ("weak", "vertex", "dup"):
        d = cs[fam]
        want = O.qp_backward(d["P"], d["q"], d["G"], d["h"], bool(normalize), w)
        ok = _non_degenerate(d["P"], d["q"], d["G"].astype(np.float32), d["h"].astype(np.float32), normalize)
        for saved in (False, True):
            got = backward(d, w, normalize, saved=saved)
            if not all(np.isfinite(got[k]).all() for k in "PqGh"):
                errs.append(f"{fam} saved={saved}: a non-finite gradient")
            e = rel(got["q"][ok], want["q"][ok])
            if not e <= 1e-5:
                errs.append(f"{fam} saved={saved}: grad_q off by {e:.3g} on {int(ok.sum())} non-degenerate lanes")
    assert not errs, "\n".join(errs)
