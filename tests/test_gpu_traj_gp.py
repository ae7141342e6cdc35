"""DynamicsModel.trajectory_rows / append_trajectory (rcbf_traj_pack_gp_f64:
k_traj_gp_count, k_traj_gp_scan, k_traj_pack_gp): the transitions of a
trajectory plan that the reference's loop hands to append_transition
(main.py:110-113), computed and compacted on the device.

The oracle is the project's own host path, already pinned to the reference: a
twin DynamicsModel (built like _dyn in tests/test_gp_host.py) whose
fit_gp_model records (history_counter, copies of both rings), driven by a
Python loop over the steps that follows main.py:110-113 literally -- rebuild
the episode step e from step0 and the done bytes, select e % every == 0,
get_state on the selected numpy rows of obs_prev and next_obs,
append_transition(x, u, x', t_batch=e * dt).  n_selected, history_counter, the
fit points and the rings at each fit and at the end must match.

Tolerances (derived, not measured):
  - cars `state` ring: bit-equal (np.array_equal).  fp32 widens exactly and
    x100 / x30 is one fp64 rounding on either side.
  - unicycle `state`: columns 0, 1 bit-equal; column 2 is atan2, ocml on the
    device against glibc on the host, each within 1 ulp of the true value near
    |theta| <= pi: 2 ulp(pi) = 2 * 2^-52 * pi apart at the most,
    doubled: atol = 4 * 2^-52 * pi = 2.8e-15.
  - `disturbance` ring: bit-equal in every column no transcendental reaches:
    for cars every column except 1 (same operations in the same order, no
    contraction, IEEE division).  Cars column 1 (sin(0.2 t) in car 0's
    acceleration) and the three unicycle columns (atan2 in x[2]; cos, sin of
    it in F) at atol = 1e-12: a 2-ulp difference in sin / cos / atan2 reaches
    d as at most about 1e-13 -- cars 40 * 2^-51 (the 10 sin term times 4, 2 ulp
    of a value <= 1) plus one rounding flip of ulp(30) * 4 in the acceleration
    and one of ulp(1) / dt in the difference; unicycle 2 * 4.4e-16 / dt from
    the two atan2 in x' - x, less in the other columns.  1e-12 is about 10x
    that bound and 1e10 below the values' scale; a larger difference is a bug.

Trajectories are synthetic (random fp32 obs, u, term_obs; done with p = 0.3;
step0 near the time limit), as in tests/test_gpu_traj_replay.py: the kernels do
not care where they come from.  One test runs a real term_obs plan.

The issue's case "K = 1, every = 2 and an odd step0: nothing selected" has the
parity backwards for its own rule (e = step0 + 1 is selected iff e % every ==
0, main.py:98,111): an EVEN step0 selects nothing.  Both parities are run."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from _traj_grid import chunk as _chunk
from test_gpu_traj_replay import DIMS, _Env, _synthetic

pytestmark = pytest.mark.gpu

N_S = {"SimulatedCars": 10, "Unicycle": 3}
ATAN_TOL = 4 * 2.0 ** -52 * math.pi
D_TOL = 1e-12
SENT = -4321.25
MARGINS = {}  # the largest difference seen per compared quantity (printed with -s)


def _dyn(mode, size=50, cuda=False, counter=0):
    """A DynamicsModel whose fit_gp_model records (counter, ring copies)."""
    from rcbf_amd.dynamics import DynamicsModel
    env = types.SimpleNamespace(dynamics_mode=mode, dt=DIMS[mode][3])
    dm = DynamicsModel(env, types.SimpleNamespace(cuda=cuda, gp_model_size=size))
    dm.history_counter = counter
    dm.snaps = []
    dm.fit_gp_model = lambda *a, **k: dm.snaps.append((dm.history_counter, dm.disturbance_history["state"].copy(),
                                                       dm.disturbance_history["disturbance"].copy()))
    return dm


def _episode_steps(traj, step0, K, auto_reset):
    """e (K, B) int64: the post-increment episode step of every transition."""
    done = traj["done"][:K].cpu().numpy() != 0
    c = step0.cpu().numpy().astype(np.int64)
    e = np.empty(done.shape, np.int64)
    for j in range(K):
        e[j] = c + 1
        c = np.where(done[j] & bool(auto_reset), 0, e[j])
    return e


def _host_loop(twin, env, traj, obs0, step0, K, every, auto_reset=True):
    """main.py:110-113 for the K steps of B envs in lock-step; returns n_selected."""
    obs, u = traj["obs"][:K].cpu().numpy(), traj["u"][:K].cpu().numpy()
    done = traj["done"][:K].cpu().numpy() != 0
    e = _episode_steps(traj, step0, K, auto_reset)
    prev, n_sel = obs0.cpu().numpy(), 0
    for j in range(K):
        nxt = obs[j].copy()
        if auto_reset:  # the terminal row, not the reset row
            nxt[done[j]] = traj["term_obs"][j].cpu().numpy()[done[j]]
        sel = e[j] % every == 0
        if sel.any():
            twin.append_transition(twin.get_state(prev[sel]), u[j][sel], twin.get_state(nxt[sel]),
                                   t_batch=e[j][sel] * env.dt)
            n_sel += int(sel.sum())
        prev = obs[j]
    return n_sel


def _note(key, val):
    MARGINS[key] = max(MARGINS.get(key, 0.0), float(val))


def _close(mode, s_a, d_a, s_b, d_b):
    """Rings (or rows) a against b, at the module docstring's tolerances."""
    assert s_a.shape == s_b.shape and d_a.shape == d_b.shape
    if s_a.size == 0:
        return
    if mode == "SimulatedCars":
        exact = [k for k in range(10) if k != 1]
        _note("cars d[1]", np.max(np.abs(d_a[:, 1] - d_b[:, 1])))
        assert np.array_equal(s_a, s_b)
        assert np.array_equal(d_a[:, exact], d_b[:, exact])
        assert np.max(np.abs(d_a[:, 1] - d_b[:, 1])) <= D_TOL
    else:
        _note("unicycle x[2]", np.max(np.abs(s_a[:, 2] - s_b[:, 2])))
        _note("unicycle d", np.max(np.abs(d_a - d_b)))
        assert np.array_equal(s_a[:, :2], s_b[:, :2])
        assert np.max(np.abs(s_a[:, 2] - s_b[:, 2])) <= ATAN_TOL
        assert np.max(np.abs(d_a - d_b)) <= D_TOL


def _same_model(mode, dm, twin):
    assert dm.history_counter == twin.history_counter
    assert [c for c, _, _ in dm.snaps] == [c for c, _, _ in twin.snaps]
    for (_, s_a, d_a), (_, s_b, d_b) in zip(dm.snaps, twin.snaps):
        _close(mode, s_a, d_a, s_b, d_b)
    _close(mode, dm.disturbance_history["state"], dm.disturbance_history["disturbance"],
           twin.disturbance_history["state"], twin.disturbance_history["disturbance"])


def _case(mode, B, P, K, every, rows=None, term=True, auto_reset=True, seed=1, size=50, counter=7, edit=None):
    env = _Env(mode, B)
    traj, obs0, step0 = _synthetic(env, K if rows is None else K + 2, P, seed)
    if edit is not None:
        edit(traj, step0)
    if not term:
        del traj["term_obs"]
    dm, twin = _dyn(mode, size, counter=counter), _dyn(mode, size, counter=counter)
    n = dm.append_trajectory(env, traj, obs0, step0, rows=rows, every=every, auto_reset=auto_reset)
    assert n == _host_loop(twin, env, traj, obs0, step0, K, every, auto_reset)
    assert dm.history_counter == counter + n
    _same_model(mode, dm, twin)
    return dm, twin, n


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    print("\nlargest differences against the host loop:", {k: f"{v:.3g}" for k, v in sorted(MARGINS.items())},
          f"(bounds: x[2] {ATAN_TOL:.3g}, d {D_TOL:.3g})")


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
@pytest.mark.parametrize("B,P", [(1, 64), (63, 64), (65, 128), (130, 192)])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("every", [1, 2, 3])
def test_ring_counter_and_fit_points_equal_the_host_loop(mode, B, P, K, every):
    """gp_model_size = 50: 130 x 5 rows wrap the ring several times and cross a
    fit point every 5 rows; the counter starts at 7."""
    _case(mode, B, P, K, every, seed=B + 7 * K + every)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_a_wave_with_no_lane_selected_and_one_with_all_64(mode):
    """Wave 0's 64 envs run in lock-step without a reset from an odd count: all
    64 selected at steps 0, 2, 4, none at steps 1, 3; wave 1 and the partial
    wave 2 stay mixed."""
    def edit(traj, step0):
        step0[:64] = 11
        traj["done"][:, :64] = 0

    env = _Env(mode, 130)
    traj, obs0, step0 = _synthetic(env, 5, 192, 3)
    edit(traj, step0)
    sel = _episode_steps(traj, step0, 5, True) % 2 == 0
    per_wave = sel[:, :64].sum(1).tolist()
    assert per_wave == [64, 0, 64, 0, 64] and 0 < sel[0, 64:128].sum() < 64
    _case(mode, 130, 192, 5, 2, seed=3, edit=edit)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_one_step_selects_nothing_or_everything_by_the_parity_of_step0(mode):
    """K = 1, every = 2.  An even step0 (e odd): nothing selected, nothing
    written, the counter unchanged.  An odd step0: every env selected."""
    def even(traj, step0):
        step0.fill_(10)

    def odd(traj, step0):
        step0.fill_(11)

    dm, _, n = _case(mode, 65, 128, 1, 2, edit=even)
    assert n == 0 and dm.history_counter == 7 and not dm.snaps
    assert not dm.disturbance_history["state"].any() and not dm.disturbance_history["disturbance"].any()
    env = _Env(mode, 65)
    traj, obs0, step0 = _synthetic(env, 1, 128, 1)
    even(traj, step0)
    state, dist, n_sel = _dyn(mode).trajectory_rows(env, traj, obs0, step0)
    assert n_sel == 0 and tuple(state.shape) == (0, N_S[mode]) == tuple(dist.shape)
    _, _, n = _case(mode, 65, 128, 1, 2, edit=odd)
    assert n == 65


def test_auto_reset_false_with_and_without_term_obs_and_rows_below_the_length():
    _case("SimulatedCars", 65, 128, 5, 2, term=False, auto_reset=False)
    _case("Unicycle", 65, 128, 5, 2, term=False, auto_reset=False)
    _case("SimulatedCars", 65, 128, 5, 2, auto_reset=False)  # term_obs present, ignored
    _case("Unicycle", 65, 128, 5, 3, auto_reset=False)
    _case("SimulatedCars", 65, 128, 5, 2, rows=5)  # arrays of 7 rows
    _case("Unicycle", 65, 128, 3, 1, rows=3)
    env = _Env("SimulatedCars", 4)
    traj, obs0, step0 = _synthetic(env, 2, 64, 5)
    del traj["term_obs"]
    with pytest.raises(ValueError, match="term_obs"):
        _dyn("SimulatedCars").trajectory_rows(env, traj, obs0, step0)


def _raw(env, traj, obs0, step0, K, every, keep_last, alloc, auto_reset=1):
    """rcbf_traj_pack_gp_f64 itself, into sentinel-filled arrays of `alloc` rows."""
    from rcbf_amd import _lib
    lib = _lib.load()
    B, n_s = env.num_envs, N_S[env.dynamics_mode]
    state = torch.full((alloc, n_s), SENT, dtype=torch.float64, device="cuda")
    dist = torch.full((alloc, n_s), SENT, dtype=torch.float64, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    nbytes = lib.rcbf_traj_pack_gp_scratch_bytes(B, K)
    assert nbytes == 8 * ((B + 63) // 64 * K + 1)
    scratch = torch.full((nbytes // 8 + 1,), 77, dtype=torch.int64, device="cuda")
    pitch = traj["obs"].stride(0) // env.n_o
    rc = lib.rcbf_traj_pack_gp_f64(_lib.ptr(state), _lib.ptr(dist), _lib.ptr(count), _lib.ptr(scratch), B, K, pitch,
                                   env.n_o, env.n_u, _lib.ptr(obs0), _lib.ptr(step0), _lib.ptr(traj["obs"]),
                                   _lib.ptr(traj.get("term_obs")), _lib.ptr(traj["u"]), _lib.ptr(traj["done"]),
                                   float(env.dt), auto_reset, every, keep_last, _lib.stream_of(torch.device("cuda", 0)))
    assert rc == 0
    torch.cuda.synchronize()
    assert scratch[-1].item() == 77  # nothing past the scratch the library asked for
    return state, dist, count.tolist()


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_keep_last_is_the_tail_of_the_unlimited_result_and_the_rest_stays_untouched(mode):
    """B = 130, K = 5, every = 2 selects a few hundred rows.  keep_last below,
    at and above a wave's 64, far below (1) and above n_sel: rows [0, rows
    written) are the last rows of the unlimited result bit for bit, every row
    after them keeps the sentinel, count_out = {n_sel, rows written}."""
    env = _Env(mode, 130)
    traj, obs0, step0 = _synthetic(env, 5, 192, 17)
    alloc = 130 * 3 + 3
    full_s, full_d, (n_sel, n_full) = _raw(env, traj, obs0, step0, 5, 2, 130 * 3, alloc)
    assert n_sel == n_full == int((_episode_steps(traj, step0, 5, True) % 2 == 0).sum()) > 130
    assert bool((full_s[n_sel:] == SENT).all()) and bool((full_d[n_sel:] == SENT).all())
    assert bool((full_s[:n_sel] != SENT).all())
    dm = _dyn(mode)
    for keep in (1, 63, 64, 65, 129, 130, n_sel - 1, n_sel, n_sel + 1):
        s, d, (ns, n) = _raw(env, traj, obs0, step0, 5, 2, keep, alloc)
        assert ns == n_sel and n == min(keep, n_sel)
        assert torch.equal(s[:n].view(torch.int64), full_s[n_sel - n:n_sel].view(torch.int64)), keep
        assert torch.equal(d[:n].view(torch.int64), full_d[n_sel - n:n_sel].view(torch.int64)), keep
        assert bool((s[n:] == SENT).all()) and bool((d[n:] == SENT).all()), keep
        ts, td, tn = dm.trajectory_rows(env, traj, obs0, step0, keep_last=keep)
        assert tn == n_sel and ts.shape[0] == n == td.shape[0]
        assert torch.equal(ts.view(torch.int64), s[:n].view(torch.int64))
        assert torch.equal(td.view(torch.int64), d[:n].view(torch.int64))
    # the unlimited rows are the host loop's, in its order (a ring that holds them all, no wrap)
    twin = _dyn(mode, size=1000)
    assert _host_loop(twin, env, traj, obs0, step0, 5, 2) == n_sel
    _close(mode, full_s[:n_sel].cpu().numpy(), full_d[:n_sel].cpu().numpy(),
           twin.disturbance_history["state"][:n_sel], twin.disturbance_history["disturbance"][:n_sel])


def _rows_against_the_host_loop(mode, B, P, K, every, seed):
    """The unlimited rows of rcbf_traj_pack_gp_f64 against the host loop's, in
    its order (a ring that holds them all, no fit); returns what a keep_last
    sweep needs."""
    env = _Env(mode, B)
    traj, obs0, step0 = _synthetic(env, K, P, seed)
    n_max = B * -(-K // every)
    full_s, full_d, (n_sel, n_full) = _raw(env, traj, obs0, step0, K, every, n_max, n_max + 3)
    sel = _episode_steps(traj, step0, K, True) % every == 0
    assert n_sel == n_full == int(sel.sum())
    assert bool((full_s[n_sel:] == SENT).all()) and bool((full_d[n_sel:] == SENT).all())
    twin = _dyn(mode, size=(n_sel // 10 + 1) * 10)  # a multiple of 10: append_transition writes whole slices
    twin.fit_gp_model = lambda *a, **k: None
    assert _host_loop(twin, env, traj, obs0, step0, K, every) == n_sel
    _close(mode, full_s[:n_sel].cpu().numpy(), full_d[:n_sel].cpu().numpy(),
           twin.disturbance_history["state"][:n_sel], twin.disturbance_history["disturbance"][:n_sel])
    return env, traj, obs0, step0, sel, full_s, full_d, n_sel


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
@pytest.mark.parametrize("every", [2, 3])
def test_several_steps_per_workgroup_equal_the_host_loop(mode, every):
    """The shapes above give every workgroup ONE step (waves x K is far below
    8 waves per CU).  B = 8 256 (129 waves) at pitch 8 320, K = 40: on a 256-CU
    device 16 parts of 3 steps, the last of 1 -- the carried row and step count
    (through resets, p = 0.3), the walk to a chunk's first step past 16 done
    bytes, the scan over 5 160 counts."""
    B, K = 8256, 40
    assert 1 < _chunk(B, K) < K and K % _chunk(B, K)
    _rows_against_the_host_loop(mode, B, 8320, K, every, seed=41 + every)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_the_flagship_grid_ten_steps_per_workgroup(mode):
    """B = 65 600 (1 025 waves, the last of 32 envs), K = 19: two parts, of 10
    and 9 steps on a 256-CU device, so the count pass runs a full batch of 8
    done bytes and a tail in each."""
    B, K = 65600, 19
    assert _chunk(B, K) > 8
    _rows_against_the_host_loop(mode, B, 65664, K, 2, seed=57)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_keep_last_cuts_inside_a_chunk_of_several_steps(mode):
    """B = 8 256, K = 40, every = 2 (chunks of 3 steps): the first kept row
    falls inside a step in the middle of a chunk, on a chunk's first and last
    step, on a step's first row, inside the one-step last chunk, and keeps a
    single row: rows [0, rows written) are the tail of the unlimited result bit
    for bit, the rows after them keep the sentinel."""
    B, K = 8256, 40
    chunk = _chunk(B, K)
    assert 1 < chunk < K
    env, traj, obs0, step0, sel, full_s, full_d, n_sel = _rows_against_the_host_loop(mode, B, 8320, K, 2, seed=43)
    cum = np.concatenate([[0], np.cumsum(sel.sum(1))])  # selected rows before step j
    mid, last = chunk + chunk // 2, K - 1
    skips = [int(cum[mid]) + 100, int(cum[mid]), int(cum[chunk]) + 64 + 7, int(cum[2 * chunk - 1]) + 4000,
             int(cum[last]) + 5, int(cum[last]) - 1, n_sel - 1]
    assert all(0 < s < n_sel for s in skips) and cum[mid + 1] - cum[mid] > 100
    for skip in skips:
        keep = n_sel - skip
        s, d, (ns, n) = _raw(env, traj, obs0, step0, K, 2, keep, keep + 3)
        assert ns == n_sel and n == keep
        assert torch.equal(s[:n].view(torch.int64), full_s[skip:n_sel].view(torch.int64)), skip
        assert torch.equal(d[:n].view(torch.int64), full_d[skip:n_sel].view(torch.int64)), skip
        assert bool((s[n:] == SENT).all()) and bool((d[n:] == SENT).all()), skip


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_refit_last_and_none_leave_the_ring_of_refit_every(mode):
    """650 rows through a 50-row ring from counter 7 (wraps 13 times), 3 rows
    that cross the fit point at 10, and 3 rows from counter 6 that cross none:
    ring and counter as refit='every' leaves them; 'last' fits once iff a fit
    point was crossed, at the final counter; 'none' never."""
    for B, K, every, counter, crossed in ((130, 5, 1, 7, True), (3, 1, 1, 8, True), (3, 1, 1, 6, False)):
        env = _Env(mode, B)
        traj, obs0, step0 = _synthetic(env, K, 192, 23)
        ref = _dyn(mode, counter=counter)
        n = ref.append_trajectory(env, traj, obs0, step0, every=every)
        assert n == B * K and (len(ref.snaps) > 0) == crossed
        for refit in ("last", "none"):
            dm = _dyn(mode, counter=counter)
            assert dm.append_trajectory(env, traj, obs0, step0, every=every, refit=refit) == n
            assert dm.history_counter == ref.history_counter == counter + n
            for f in ("state", "disturbance"):
                assert np.array_equal(dm.disturbance_history[f], ref.disturbance_history[f]), (refit, f)
            assert [c for c, _, _ in dm.snaps] == ([counter + n] if crossed and refit == "last" else [])
            if dm.snaps:  # ... on the final ring
                assert np.array_equal(dm.snaps[0][1], ref.disturbance_history["state"])


def test_term_obs_plan_into_the_gp_dataset_end_to_end():
    """Cars, B = 65, K = 310: every env ends an episode inside the plan.  The
    rows of a step that ended an episode carry the terminal row as x' (not the
    reset row), and the same env's next row starts from the reset row."""
    from rcbf_amd.aql import AqlQueue
    from test_gpu_aql_fused import _pool, _twins
    mode, B, K = "SimulatedCars", 65, 310
    (env, layer), = _twins(mode, B, n=1)
    q = AqlQueue(torch.device("cuda", 0))
    try:
        traj = env.make_trajectory(K, ("obs", "u", "reward", "done", "term_obs"))
        traj["term_obs"]._base.fill_(SENT)  # only the rows of done steps are written
        obs0, step0 = env.obs.clone(), env.step_count.clone()
        plan = q.safe_step_plan(env, _pool(env, 7), layer, steps=K, trajectory=traj)
        plan.run()
        torch.cuda.synchronize()
        size = B * K + 5  # a ring that keeps every row in order
        dm, twin = _dyn(mode, size), _dyn(mode, size)
        n = dm.append_trajectory(env, traj, obs0, step0, every=2)
        assert n == _host_loop(twin, env, traj, obs0, step0, K, 2)
        _same_model(mode, dm, twin)
        done = traj["done"].cpu().numpy() != 0
        assert done.any(0).all()
        obs, term = traj["obs"].cpu().numpy().astype(np.float64), traj["term_obs"].cpu().numpy().astype(np.float64)
        e = _episode_steps(traj, step0, K, True)
        for every in (2, 1):
            state, dist, n_sel = dm.trajectory_rows(env, traj, obs0, step0, every=every)
            x, d = state.cpu().numpy(), dist.cpu().numpy()
            sel = e % every == 0
            row = (np.cumsum(sel.ravel()) - 1).reshape(K, B)  # the row of a selected transition
            assert n_sel == sel.sum() == x.shape[0]
            # episodes end at the time limit, e = 300: selected at every = 2 and 1; those with a later step in the plan
            js, es = np.nonzero(done[:K - 2] & sel[:K - 2])
            assert js.size >= B
            r = row[js, es]
            # x' positions from the stored row: x' = x + dt (d + F), F of a position its car's velocity
            xn_pos = x[r, ::2] + 0.02 * (d[r, ::2] + x[r, 1::2])
            assert np.max(np.abs(xn_pos - 100.0 * term[js, es, ::2])) < 1e-9
            assert np.all(np.abs(xn_pos - 100.0 * obs[js, es, ::2]).max(1) > 1.0)  # ... not the reset row
            # the env's next selected row: step j + every, e = every, from the row `every - 1` steps after the reset
            nxt = row[js + every, es]
            assert np.all(sel[js + every, es]) and np.all(e[js + every, es] == every)
            assert np.array_equal(x[nxt, ::2], 100.0 * obs[js + every - 1, es, ::2])
            assert np.array_equal(x[nxt, 1::2], 30.0 * obs[js + every - 1, es, 1::2])
        plan.free()
    finally:
        q.close()


def test_one_real_fit_from_a_trajectory():
    """Unicycle, gp_model_size = 200, B = 8, K = 60, every = 2, refit='last':
    240 rows through the 200-row ring, one real GP fit at the end, and the
    fitted model predicts."""
    from rcbf_amd.dynamics import DynamicsModel
    mode, B, K = "Unicycle", 8, 60
    env = _Env(mode, B)
    traj, obs0, step0 = _synthetic(env, K, 64, 31)
    step0.fill_(1)
    traj["done"].zero_()  # lock-step: 30 selected steps of 8 envs
    for f in ("obs", "term_obs", "u"):
        traj[f].mul_(0.05)  # small motions: disturbances of order 1
    dm = DynamicsModel(types.SimpleNamespace(dynamics_mode=mode, dt=0.02),
                       types.SimpleNamespace(cuda=True, gp_model_size=200))
    assert dm.disturb_estimators is None
    assert dm.append_trajectory(env, traj, obs0, step0, every=2, refit="last") == 240 == dm.history_counter
    assert dm.disturb_estimators is not None and dm.train_x.shape == (200, 3)
    x = dm.disturbance_history["state"][:4]
    mean, std = dm.predict_disturbance(x)
    assert mean.shape == (4, 3) == std.shape and np.isfinite(mean).all() and np.isfinite(std).all() and (std > 0).all()
