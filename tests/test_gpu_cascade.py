"""The Cascade layer's kernels (csrc/rcbf_cascade.hip: rcbf_cascade_u_safe, the
device path, and rcbf_cascade_u_safe_sync, the one-workgroup pinned-memory
path of up to 256 samples) against the oracle on tests/_cascade_cases.py:
states with two and three hazard rows active at once, every hazard count
1..8, waves whose lanes need 0, 1, 2, 3 and K rows, all three solvers.

Reference: oracle.qp_exact on the oracle's own normalised rows; it solves
every row (tests/test_cascade_cases_cpu.py), so no lane is excluded anywhere.
Bars, relative to max(1, |ref|), the project's own: cars 1e-9, unicycle 1e-7
(test_cascade_golden; the fp64 'illcond' bar of test_gpu_qp_hard) on the safe
action and on the slack; rows G 1e-14, h 1e-13 (test_cascade_golden).
"""
import ctypes
import functools
import threading

import numpy as np
import pytest
import torch

import _cascade_cases as C

pytestmark = pytest.mark.gpu

CASES = tuple(C.KS) + ("cars",)
SOLVERS = (0, 1, 2)
OK, NONFINITE = 0, 3
E_BAD_SHAPE = 1002
MIX = len(C.KINDS) * C.WAVE  # first row of the waves that mix the kinds (unicycle)


def bar(name):
    return 1e-9 if name == "cars" else 1e-7


def n_u(name):
    return 1 if name == "cars" else 2


@functools.lru_cache(maxsize=None)
def layer(name, solver=0):
    from rcbf_amd.cbf_qp import CascadeCBFLayer
    from rcbf_amd.envs import SimulatedCarsEnv, UnicycleEnv
    if name == "cars":
        return CascadeCBFLayer(SimulatedCarsEnv(), gamma_b=C.CARS_GAMMA_B, k_d=C.K_D, solver=solver)
    env = UnicycleEnv()
    env.hazards_locations = np.array(C.hazards(name))
    return CascadeCBFLayer(env, gamma_b=C.GAMMA_B, k_d=C.K_D, l_p=C.L_P, solver=solver)


def args(d, sl=slice(None)):
    """(u_nom, state, mean, sigma) of rows sl, as copies: the cases are shared and read-only."""
    return tuple(np.array(d[k][sl]) for k in ("u", "x", "mu", "sigma"))


def errors(name, us, eps, sl=slice(None)):
    """(action error, slack error) against the oracle's rows sl."""
    z = C.reference(name)["z"][sl]
    return C.rel(us, z[:, :-1]), C.rel(eps, z[:, -1])


# ----------------------------------------------------------------------------
# through CascadeCBFLayer
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", CASES)
def test_forward_matches_oracle(name, solver, capsys):
    """get_u_safe and last_eps on the whole batch (the device path) and on its
    first 256 rows (the one-workgroup path)."""
    d, L = C.case(name), layer(name, solver)
    out = []
    for path, sl in (("device", slice(None)), ("sync", slice(0, 256))):
        us = L.get_u_safe(*args(d, sl))
        assert us.shape == (len(d["x"][sl]), n_u(name))
        out.append((path,) + errors(name, us, L.last_eps, sl))
    with capsys.disabled():
        print(f"\n  cascade {name} solver={solver}: " +
              ", ".join(f"{p} u {eu:.2e} eps {ee:.2e}" for p, eu, ee in out))
    for p, eu, ee in out:
        assert eu <= bar(name) and ee <= bar(name), (p, eu, ee)


@pytest.mark.parametrize("name", CASES)
def test_rows_match_oracle(name):
    d, ref = C.case(name), C.reference(name)
    P, q, G, h = layer(name).get_cbf_qp_constraints(*args(d))
    assert C.rel(G, ref["G"]) < 1e-14 and C.rel(h, ref["h"]) < 1e-13, (C.rel(G, ref["G"]), C.rel(h, ref["h"]))
    assert np.array_equal(P, np.broadcast_to(np.diag(C.pdiag(name)), P.shape)) and not q.any()


@pytest.mark.parametrize("name", [5, "cars"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257])
def test_hand_over_between_the_paths(name, B):
    """get_u_safe at the sizes around a wave and around the 256-sample switch
    from the pinned-memory path to the device path."""
    lo = MIX if name != "cars" else 0
    sl = slice(lo, lo + B)
    L = layer(name)
    us = L.get_u_safe(*args(C.case(name), sl))
    assert us.shape == (B, n_u(name)) and L.last_eps.shape == (B,)
    eu, ee = errors(name, us, L.last_eps, sl)
    assert eu <= bar(name) and ee <= bar(name), (eu, ee)


# ----------------------------------------------------------------------------
# the C-ABI directly
# ----------------------------------------------------------------------------
def call(name, d, sl=slice(None), solver=0, status=True, flag=0, eps=True, null_prior=False):
    """One launch of rcbf_cascade_u_safe on rows sl of d.  The outputs carry
    one guard row past the batch.  Returns dict(u, eps, st, flag, guards)."""
    from rcbf_amd import _lib
    lib = _lib.load()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda").contiguous()
    U, X, M, S = (t(a) for a in args(d, sl))
    B = X.shape[0]
    out = torch.full((B + 1, n_u(name)), 12345.0, dtype=torch.float64, device="cuda")
    e = torch.full((B + 1,), 12345.0, dtype=torch.float64, device="cuda") if eps else None
    st = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda") if status else None
    fl = torch.tensor([flag], dtype=torch.int32, device="cuda") if flag is not None else None
    rc = lib.rcbf_cascade_u_safe(ctypes.byref(layer(name, solver)._prm), B, _lib.ptr(U), _lib.ptr(X),
                                 None if null_prior else _lib.ptr(M), None if null_prior else _lib.ptr(S),
                                 _lib.ptr(out), _lib.ptr(st), _lib.ptr(fl), _lib.ptr(e), _lib.stream_of(out.device))
    assert rc == 0
    torch.cuda.synchronize()
    out, e, st = (None if v is None else v.cpu().numpy() for v in (out, e, st))
    guards = (out[B] == 12345.0).all() and (e is None or e[B] == 12345.0) and (st is None or st[B] == -7)
    return dict(u=out[:B], eps=None if e is None else e[:B], st=None if st is None else st[:B],
                flag=None if fl is None else int(fl.item()), guards=bool(guards))


@pytest.mark.parametrize("name", CASES)
def test_reporting_outputs_do_not_change_the_action(name):
    """status_out, fail_flag and eps_out, each present and absent: u_safe_out
    bit for bit the same, status 0 on every lane, the flag untouched."""
    d = C.case(name)
    base = call(name, d)
    assert base["guards"] and (base["st"] == OK).all() and base["flag"] == 0
    eu, ee = errors(name, base["u"], base["eps"])
    assert eu <= bar(name) and ee <= bar(name), (eu, ee)
    for status in (True, False):
        for flag in (0, None):
            for eps in (True, False):
                o = call(name, d, status=status, flag=flag, eps=eps)
                tag = (status, flag, eps)
                assert o["guards"], tag
                assert o["u"].tobytes() == base["u"].tobytes(), tag
                assert o["eps"] is None or o["eps"].tobytes() == base["eps"].tobytes(), tag
                assert o["st"] is None or (o["st"] == OK).all(), tag
                assert o["flag"] in (0, None), tag
    assert call(name, d, flag=1 << 30)["flag"] == 1 << 30  # bits already set stay, none is added


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", CASES)
def test_null_mean_and_sigma_are_the_prior(name, solver):
    """mu = sigma = NULL: bit-equal to zeros and float64(float32(0.2)) (0 on
    the cars positions), what prior_sigma yields."""
    d = dict(C.case(name))
    d["mu"] = np.zeros_like(d["x"])
    d["sigma"] = np.full_like(d["x"], np.float64(np.float32(0.2)))
    if name == "cars":
        d["sigma"][:, 0::2] = 0.0
    a, b = call(name, d, solver=solver), call(name, d, solver=solver, null_prior=True)
    assert a["u"].tobytes() == b["u"].tobytes() and a["eps"].tobytes() == b["eps"].tobytes()
    assert (b["st"] == OK).all() and b["flag"] == 0 and b["guards"]
    z = C.solve(name, d)
    assert (z["status"] == 0).all()
    assert C.rel(b["u"], z["z"][:, :-1]) <= bar(name) and C.rel(b["eps"], z["z"][:, -1]) <= bar(name)


@pytest.mark.parametrize("name", CASES)
def test_batch_sizes_device_path(name):
    """rcbf_cascade_u_safe at B around a wave and a workgroup: the lanes past
    the batch leave before the wave's ballots and write nothing."""
    d = C.case(name)
    lo = MIX if name != "cars" else 0
    for B in (1, 63, 64, 65, 255, 256, 257):
        sl = slice(lo, lo + B)
        o = call(name, d, sl)
        eu, ee = errors(name, o["u"], o["eps"], sl)
        assert eu <= bar(name) and ee <= bar(name), (B, eu, ee)
        assert (o["st"] == OK).all() and o["flag"] == 0 and o["guards"], B


def sync_call(L, B, null_prior=False):
    """rcbf_cascade_u_safe_sync on the calling thread's staging block as it
    stands, with the next sequence number (kept only if the call ran)."""
    from rcbf_amd import _lib
    st = L._staging(1, *((10, 1) if L.env.dynamics_mode == "SimulatedCars" else (3, 2)))
    seq = (st["seq"] + 1) & 0xFFFFFFFF or 1
    rc = _lib.load().rcbf_cascade_u_safe_sync(ctypes.byref(L._prm), B, st["pu"], st["px"],
                                              None if null_prior else st["pm"], None if null_prior else st["ps"],
                                              st["po"], st["pst"], st["pe"], st["pw"], seq,
                                              _lib.stream_of(torch.cuda.current_device()))
    if rc == 0:
        st["seq"] = seq
    return rc, st


@pytest.mark.parametrize("name", [5, "cars"])
def test_null_prior_on_the_one_workgroup_path(name):
    """rcbf_cascade_u_safe_sync with mu = sigma = NULL on the inputs already in
    the staging block: bit-equal to the explicit prior."""
    d = dict(C.case(name))
    d["mu"] = np.zeros_like(d["x"])
    d["sigma"] = np.full_like(d["x"], np.float64(np.float32(0.2)))
    if name == "cars":
        d["sigma"][:, 0::2] = 0.0
    L, B = layer(name), 200
    lo = MIX if name != "cars" else 0
    us = L.get_u_safe(*args(d, slice(lo, lo + B)))
    eps = L.last_eps
    rc, st = sync_call(L, B, null_prior=True)
    assert rc == 0 and (st["status"][:B] == OK).all()
    assert st["o"][:B * n_u(name)].tobytes() == us.tobytes() and st["e"][:B].tobytes() == eps.tobytes()


@pytest.mark.parametrize("name", [3, "cars"])
def test_sync_refuses_bad_sizes(name):
    L = layer(name)
    L.get_u_safe(*args(C.case(name), slice(0, 2)))  # the staging block exists and holds valid inputs
    for B in (0, 257, -1):
        assert sync_call(L, B)[0] == E_BAD_SHAPE, B
    us = L.get_u_safe(*args(C.case(name), slice(0, 2)))  # and the layer still works
    assert errors(name, us, L.last_eps, slice(0, 2))[0] <= bar(name)


# ----------------------------------------------------------------------------
# one NaN state among clean lanes
# ----------------------------------------------------------------------------
NAN_LANE = 17


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_nan_lane_in_the_far_wave(K, solver):
    """Lane 17 of the all-far wave gets a NaN position: its live-row mask is
    full (a NaN row is kept), so the wave's ballot sends all 64 lanes, whose
    own count is 0, to the K-slot solve.  That lane alone reports
    RCBF_QP_NONFINITE and a NaN action; the flag is exactly 1 << 3.  The
    general solvers (1, 2) report the same on the same inputs (Goldfarb-Idnani
    used to leave its start point, z = -0, on that lane: cascade_one now
    writes NaN whatever the solver)."""
    d = dict(C.case(K))
    d["x"] = d["x"].copy()
    d["x"][NAN_LANE, 0] = np.nan
    clean = np.arange(C.UNI_B) != NAN_LANE
    o = call(K, d, solver=solver)
    assert o["guards"]
    assert o["st"][NAN_LANE] == NONFINITE and np.isnan(o["u"][NAN_LANE]).all() and np.isnan(o["eps"][NAN_LANE])
    assert (o["st"][clean] == OK).all() and o["flag"] == 1 << NONFINITE
    z = C.reference(K)["z"]
    assert C.rel(o["u"][clean], z[clean, :2]) <= bar(K) and C.rel(o["eps"][clean], z[clean, 2]) <= bar(K)


@pytest.mark.parametrize("name", [5, "cars"])
def test_nan_state_raises_and_the_next_call_is_clean(name):
    """Through get_u_safe: quadprog's ValueError on both paths (B = 3 and
    B = 300), and the next clean call on that path is correct."""
    d = dict(C.case(name))
    d["x"] = d["x"].copy()
    d["x"][1, 6 if name == "cars" else 0] = np.nan  # a position the rows read (car 4's; the unicycle's x)
    L = layer(name)
    lo = MIX if name != "cars" else 0
    for B in (3, 300):
        with pytest.raises(ValueError):
            L.get_u_safe(*args(d, slice(0, B)))
        sl = slice(lo, lo + B)
        us = L.get_u_safe(*args(C.case(name), sl))
        eu, ee = errors(name, us, L.last_eps, sl)
        assert eu <= bar(name) and ee <= bar(name), (B, eu, ee)


# ----------------------------------------------------------------------------
# the pinned-memory path's state
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [5, "cars"])
def test_sequence_word_wraps(name):
    """Four calls across the wrap of the completion sequence (0xFFFFFFFF, then
    1: 0 is skipped, it is the word's initial value), each on other rows."""
    L, d = layer(name), C.case(name)
    L.get_u_safe(*args(d, slice(0, 1)))
    st = L._staging(1, d["x"].shape[1], n_u(name))
    st["seq"] = 0xFFFFFFFE
    seqs = []
    lo = MIX if name != "cars" else 0
    for i, B in enumerate((5, 256, 1, 64)):
        sl = slice(lo + 7 * i, lo + 7 * i + B)
        us = L.get_u_safe(*args(d, sl))
        seqs.append(st["seq"])
        eu, ee = errors(name, us, L.last_eps, sl)
        assert eu <= bar(name) and ee <= bar(name), (i, eu, ee)
        assert ctypes.c_uint32.from_address(st["pw"]).value == st["seq"]
    assert seqs == [0xFFFFFFFF, 1, 2, 3]


@pytest.mark.parametrize("name", [5, "cars"])
def test_two_threads_on_one_layer(name):
    """Two threads, 32 single-sample calls each, on one layer (a staging block
    and a completion word per thread): every result bit-equal to the same
    call made alone."""
    L, d = layer(name), C.case(name)
    lo = MIX if name != "cars" else 0
    rows = [[lo + 2 * i + t for i in range(32)] for t in range(2)]
    alone = {}
    for r in rows[0] + rows[1]:
        u = L.get_u_safe(d["u"][r], d["x"][r], d["mu"][r], d["sigma"][r])
        alone[r] = (u.tobytes(), L.last_eps.tobytes())
        assert u.shape == (n_u(name),)
    got, errs = [{}, {}], []
    start = threading.Barrier(2, timeout=30)

    def work(t):
        try:
            start.wait()
            st = L._staging(1, d["x"].shape[1], n_u(name))  # this thread's block
            for r in rows[t]:
                u = L.get_u_safe(d["u"][r], d["x"][r], d["mu"][r], d["sigma"][r])
                got[t][r] = (u.tobytes(), st["e"][:1].tobytes())  # last_eps is the layer's: the other thread's too
        except BaseException as e:  # reported by the main thread
            errs.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads), "a thread stalled in get_u_safe"
    assert not errs, errs
    assert len(L._stages) >= 3  # the main thread's block and one per worker
    for t in range(2):
        assert got[t] == {r: alone[r] for r in rows[t]}, t
