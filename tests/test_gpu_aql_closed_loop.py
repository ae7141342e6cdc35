"""Closed-loop AQL plans (rcbf_aql_closed_loop_plan, AqlQueue.closed_loop_plan):
2K packets, the policy's kernel (rcbf::k_policy_step) before every safe step.

The oracle is the launch loop that exists without them: on a twin env, K times
policy.act(env.obs, evaluate, counter=c + j, out=u) then
env.safe_step(u, layer, outputs=o) through the HIP launch path, the outputs
cloned after every step.  Both paths run the same arithmetic in the same
order (the policy kernels share one body, the step kernels are the same machine
code), so every comparison is equality of bytes: no tolerance anywhere.

B = 65: a full wave plus one lane for the step, three 32-row policy tiles with
a ragged last one.  H = 64 from the fixture unless a test says otherwise.
"""
import ctypes

import numpy as np
import pytest
import torch

import _policy_port as PP
from test_gpu_aql_trajectory import SENTINEL
from test_gpu_policy import Args, _make_env, _tile_threshold, case

pytestmark = pytest.mark.gpu

B, K = 65, 12
TIMEOUT_US = 5_000_000
E_BAD_MODE, E_BAD_SHAPE = 1001, 1002
STEP_FIELDS = ("u", "reward", "cost", "done", "goal_met")


@pytest.fixture(scope="module")
def queue():
    from rcbf_amd.aql import AqlQueue
    q = AqlQueue(torch.device("cuda", 0), profile=True)
    yield q
    q.close()


def _same(a, b):
    """Equal as bytes (NaN payloads and signed zeros included)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _preload(env):
    """Step counts a few steps before the time limit, a different one per env: envs 0, 8, 16, ... end their
    episode inside 12 steps."""
    n = env.num_envs
    env.load_state(step=env.max_episode_steps - 2 - (np.arange(n) * 7) % 55)


def _twins(name, n=2, batch=B, seed=21, **layer_kw):
    out = []
    for _ in range(n):
        env, layer = _make_env(name, batch, seed=seed)
        if layer_kw:
            from rcbf_amd.diff_cbf_qp import CBFQPLayer
            layer = CBFQPLayer(env, Args(), gamma_b=20.0, **layer_kw)
        _preload(env)
        out.append((env, layer))
    return out


def _launch_loop(env, layer, pol, steps, evaluate, c0, o):
    """The reference: `steps` times act + safe_step; [{field: clone}] per step, "u_rl" the policy's action."""
    u = torch.empty(env.num_envs, env.n_u, dtype=torch.float32, device="cuda")
    rows = []
    for j in range(steps):
        pol.act(env.obs, evaluate=evaluate, counter=c0 + j, out=u)
        env.safe_step(u, layer, outputs=o)
        rows.append({"obs": env.obs.clone(), "u_rl": u.clone(), **{f: o[f].clone() for f in STEP_FIELDS}})
    return rows


def _assert_rows(traj, rows, steps, first=0):
    for j in range(steps):
        for f, t in traj.items():
            if f in rows[first + j]:
                assert _same(t[j], rows[first + j][f]), (f, j)


def _assert_state(e1, o1, e2, o2):
    for f in ("x", "aux", "step_count", "episode", "obs"):
        assert _same(getattr(e1, f), getattr(e2, f)), f
    for f in STEP_FIELDS:
        assert _same(o1[f], o2[f]), f


@pytest.mark.parametrize("evaluate", [True, False], ids=["evaluate", "sample"])
@pytest.mark.parametrize("name", ["cars", "unicycle"])
def test_plan_equals_the_launch_loop(golden, queue, name, evaluate):
    pol = case(golden, name, 64)[5]
    (e1, l1), (e2, l2) = _twins(name)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    c0 = 1000
    rows = _launch_loop(e1, l1, pol, K, evaluate, c0, o1)
    plan = queue.closed_loop_plan(e2, pol, l2, K, evaluate=evaluate, outputs=o2, trajectory=True)
    assert plan.dispatches == 2 * K and plan.K == K
    assert set(plan.trajectory) == set(e2.TRAJECTORY_FIELDS)
    before = pol._counter
    if evaluate:
        plan.run(timeout_us=TIMEOUT_US)
    else:
        plan.run(counter=c0, timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    assert pol._counter == before  # an explicit counter (and an evaluation plan) leaves the policy's alone
    _assert_rows(plan.trajectory, rows, K)
    assert _same(plan.u_rl, rows[K - 1]["u_rl"])
    _assert_state(e1, o1, e2, o2)
    done = plan.trajectory["done"].cpu().numpy()
    assert int(done.any(0).sum()) >= 3, "several envs end an episode inside the plan"
    assert int(e2.episode.max()) >= 1
    e1.check_failures()
    e2.check_failures()
    plan.free()


def test_second_run_continues_and_advances_the_policy_counter(golden, queue):
    pol = case(golden, "unicycle", 64)[5]
    (e1, l1), (e2, l2) = _twins("unicycle")
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    c0 = pol._counter = 77
    rows = _launch_loop(e1, l1, pol, 2 * K, False, c0, o1)
    assert pol._counter == c0  # act() with an explicit counter
    plan = queue.closed_loop_plan(e2, pol, l2, K, evaluate=False, outputs=o2, trajectory=True)
    for r in range(2):
        plan.run(timeout_us=TIMEOUT_US)
        torch.cuda.synchronize()
        assert pol._counter == c0 + (r + 1) * K
        _assert_rows(plan.trajectory, rows, K, first=r * K)
        assert _same(plan.u_rl, rows[(r + 1) * K - 1]["u_rl"])
    _assert_state(e1, o1, e2, o2)
    # the draws differ from step to step and from run to run: a stuck counter would repeat them
    assert not _same(rows[0]["u_rl"], rows[K]["u_rl"])
    plan.free()


def test_copy_back_false_still_returns_the_observation(golden, queue):
    """Two runs with copy_back=False and sync_hip=False (after a synchronise): the second run's first policy
    packet reads env.obs, which the first run must have left there."""
    pol = case(golden, "cars", 64)[5]
    (e1, l1), (e2, l2) = _twins("cars")
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    rows = _launch_loop(e1, l1, pol, 2 * K, False, 5, o1)
    plan = queue.closed_loop_plan(e2, pol, l2, K, evaluate=False, outputs=o2, trajectory=True)
    for r in range(2):
        torch.cuda.synchronize()
        plan.run(counter=5 + r * K, sync_hip=False, timeout_us=TIMEOUT_US, copy_back=False)
        torch.cuda.synchronize()
        _assert_rows(plan.trajectory, rows, K, first=r * K)
        assert _same(e2.obs, rows[(r + 1) * K - 1]["obs"])
    plan.free()


def test_plain_plan_without_a_trajectory(golden, queue):
    """No recorded field: every policy packet after the first reads the one observation buffer."""
    pol = case(golden, "unicycle", 64)[5]
    (e1, l1), (e2, l2) = _twins("unicycle")
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    rows = _launch_loop(e1, l1, pol, K, True, 0, o1)
    plan = queue.closed_loop_plan(e2, pol, l2, K, evaluate=True, outputs=o2)
    assert plan.trajectory is None and plan.dispatches == 2 * K
    plan.run(timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    assert _same(plan.u_rl, rows[K - 1]["u_rl"])
    _assert_state(e1, o1, e2, o2)
    plan.free()


@pytest.mark.parametrize("name", ["cars", "unicycle"])
def test_term_obs_is_the_open_loop_plans(golden, queue, name):
    """The launch loop's actions (bit-equal to the plan's by the first test) fed to the existing open-loop
    trajectory plan with term_obs on a third env: the closed-loop plan's term_obs equals that array where done
    is set and keeps the sentinel everywhere else."""
    pol = case(golden, name, 64)[5]
    (e1, l1), (e2, l2), (e3, l3) = _twins(name, n=3)
    o1, o2, o3 = e1.make_outputs(), e2.make_outputs(), e3.make_outputs()
    rows = _launch_loop(e1, l1, pol, K, True, 0, o1)
    fields = e2.TRAJECTORY_FIELDS + ("term_obs",)
    t2, t3 = e2.make_trajectory(K + 1, fields), e3.make_trajectory(K + 1, fields)
    for t in (t2, t3):
        t["term_obs"]._base.fill_(SENTINEL[torch.float32])
    closed = queue.closed_loop_plan(e2, pol, l2, K, evaluate=True, outputs=o2, trajectory=t2)
    assert closed.dispatches == 2 * K
    closed.run(timeout_us=TIMEOUT_US)
    opened = queue.safe_step_plan(e3, [r["u_rl"] for r in rows], l3, steps=K, outputs=o3, trajectory=t3)
    assert opened.dispatches == 1
    opened.run(timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    _assert_rows({f: t for f, t in t2.items() if f != "term_obs"}, rows, K)
    _assert_state(e1, o1, e2, o2)
    done = t2["done"][:K].bool()
    assert int(done.sum()) >= 3, "envs end an episode inside the run"
    assert _same(t2["term_obs"]._base, t3["term_obs"]._base)
    term = t2["term_obs"][:K]
    sent = term == SENTINEL[torch.float32]
    assert bool(sent[~done].all()) and not bool(sent[done].all(-1).any())
    assert bool((t2["term_obs"]._base[K:] == SENTINEL[torch.float32]).all())
    assert bool((t2["term_obs"]._base[:, B:] == SENTINEL[torch.float32]).all())
    closed.free()
    opened.free()


@pytest.mark.parametrize("evaluate", [True, False], ids=["evaluate", "sample"])
@pytest.mark.parametrize("tiles", ["32-row", "64-row"])
def test_large_lds_in_the_packet(golden, queue, tiles, evaluate):
    """H = 256: the policy packet carries 68 096 B of LDS at B = 65 (32-row tiles) and 136 192 B at
    B = 32 x CUs + 1 (64-row tiles) -- above the 64 KiB a dispatch gets without asking, and nothing but the
    packet's own group_segment_size asks.  K = 2, cars."""
    pol = case(golden, "cars", 256)[5]
    n = B if tiles == "32-row" else _tile_threshold() + 1
    (e1, l1), (e2, l2) = _twins("cars", batch=n)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    rows = _launch_loop(e1, l1, pol, 2, evaluate, 31, o1)
    plan = queue.closed_loop_plan(e2, pol, l2, 2, evaluate=evaluate, outputs=o2, trajectory=True)
    assert plan.dispatches == 4
    plan.run(timeout_us=TIMEOUT_US, **({} if evaluate else {"counter": 31}))
    torch.cuda.synchronize()
    _assert_rows(plan.trajectory, rows, 2)
    assert _same(plan.u_rl, rows[1]["u_rl"])
    _assert_state(e1, o1, e2, o2)
    plan.free()


def test_refresh_is_seen_by_the_next_run(golden, queue):
    from rcbf_amd.policy import DevicePolicy
    sd, scale, bias = case(golden, "cars", 64)[:3]
    module = PP.torch_module(sd, scale, bias).to("cuda")
    pol = DevicePolicy(module)
    (e1, l1), (e2, l2) = _twins("cars")
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    start = {f: getattr(e1, f).clone() for f in ("x", "aux", "step_count", "episode", "obs")}
    plan = queue.closed_loop_plan(e2, pol, l2, K, evaluate=True, outputs=o2, trajectory=True)
    rows = _launch_loop(e1, l1, pol, K, True, 0, o1)
    plan.run(timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    _assert_rows(plan.trajectory, rows, K)
    first_u = plan.u_rl.clone()
    with torch.no_grad():
        module.mean_linear.bias.add_(0.25)
        module.linear2.weight.mul_(0.5)
    ptr = pol.packed.data_ptr()
    pol.refresh()
    assert pol.packed.data_ptr() == ptr
    for e in (e1, e2):  # both from the first run's start: only the weights differ
        for f, t in start.items():
            getattr(e, f).copy_(t)
    rows2 = _launch_loop(e1, l1, pol, K, True, 0, o1)
    plan.run(timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    _assert_rows(plan.trajectory, rows2, K)
    assert _same(plan.u_rl, rows2[K - 1]["u_rl"])
    _assert_state(e1, o1, e2, o2)
    assert not _same(plan.u_rl, first_u) and not _same(rows2[0]["u_rl"], rows[0]["u_rl"])
    plan.free()


@pytest.mark.parametrize("chunk", [16, None])
@pytest.mark.parametrize("name", ["cars", "unicycle"])
def test_evaluate_policy_on_a_queue_is_evaluate_policy(golden, queue, name, chunk):
    """60 steps from the preloaded step counts (every env's episode ends inside the run): chunk = 16 is three
    full plans and a ragged one, chunk = None one plan of 60."""
    from rcbf_amd.evaluator import _evaluate_from, _evaluate_plans
    pol = case(golden, name, 64)[5]
    (e1, l1), (e2, l2) = _twins(name)
    want = _evaluate_from(e1, pol, l1, 60)
    got = _evaluate_plans(e2, pol, l2, 60, queue=queue, chunk=chunk)
    assert list(got) == list(want)
    assert got["episodes"] == want["episodes"] == B
    for f in ("reward", "cost", "length"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert got[f].tobytes() == want[f].tobytes(), f
    for f in ("avg_reward", "avg_cost"):
        assert type(got[f]) is float and np.float64(got[f]).tobytes() == np.float64(want[f]).tobytes(), f
    for f in ("x", "aux", "step_count", "episode", "obs"):
        assert _same(getattr(e1, f), getattr(e2, f)), f


def test_evaluate_policy_public_call_with_a_queue(golden, queue):
    """From a reset, one whole cars episode: 300 steps are a plan of 256 and a ragged one of 44."""
    from rcbf_amd.evaluator import evaluate_policy
    pol = case(golden, "cars", 64)[5]
    (e1, l1), (e2, l2) = _twins("cars")
    want = evaluate_policy(e1, pol, l1, steps=300)
    got = evaluate_policy(e2, pol, l2, steps=300, queue=queue)
    assert got["episodes"] == want["episodes"] == B
    for f in ("reward", "cost", "length"):
        assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), f
    assert got["avg_reward"] == want["avg_reward"] and got["avg_cost"] == want["avg_cost"]
    with pytest.raises(ValueError, match="chunk"):
        evaluate_policy(e2, pol, l2, steps=10, chunk=4)
    with pytest.raises(ValueError, match="chunk"):
        evaluate_policy(e2, pol, l2, steps=10, queue=queue, chunk=0)


def _valid_plan_still_runs(queue, pol, env, layer):
    plan = queue.closed_loop_plan(env, pol, layer, 2, evaluate=True)
    plan.run(timeout_us=TIMEOUT_US)
    torch.cuda.synchronize()
    env.check_failures()
    plan.free()


def test_refusals(golden, queue):
    from rcbf_amd import _lib, aql
    from rcbf_amd.policy import DevicePolicy
    pol = case(golden, "cars", 64)[5]
    uni = case(golden, "unicycle", 64)[5]
    (e1, l1), = _twins("cars", n=1)
    with pytest.raises(ValueError, match="observations"):
        queue.closed_loop_plan(e1, uni, l1, K, evaluate=True)
    _valid_plan_still_runs(queue, pol, e1, l1)
    sd, scale, bias = case(golden, "cars", 64)[:3]
    module = PP.torch_module(sd, scale, bias).to("cuda")
    del module.log_std_linear
    headless = DevicePolicy(module)
    with pytest.raises(NotImplementedError, match="log-std"):
        queue.closed_loop_plan(e1, headless, l1, K, evaluate=False)
    queue.closed_loop_plan(e1, headless, l1, K, evaluate=True).free()  # the mean alone needs no such head
    _valid_plan_still_runs(queue, pol, e1, l1)
    for flags in (aql.PROFILE, 8, 16, 32):  # per-dispatch timestamps, the study fences
        with pytest.raises(ValueError, match="profile"):
            queue.closed_loop_plan(e1, pol, l1, K, evaluate=True, fence_flags=flags)
    _valid_plan_still_runs(queue, pol, e1, l1)
    (e2, l2), = _twins("cars", n=1, solver=_lib.SOLVER_PDIPM)
    with pytest.raises(ValueError, match="solver"):
        queue.closed_loop_plan(e2, pol, l2, K, evaluate=True, trajectory=e2.make_trajectory(K, ("done", "term_obs")))
    _valid_plan_still_runs(queue, pol, e2, l2)  # PDIPM steps without term_obs are fine
    with pytest.raises(ValueError, match="DevicePolicy"):
        queue.closed_loop_plan(e1, module, l1, K, evaluate=True)
    with pytest.raises(ValueError, match="steps"):
        queue.closed_loop_plan(e1, pol, l1, 0, evaluate=True)
    plan = queue.closed_loop_plan(e1, pol, l1, 2, evaluate=True)
    with pytest.raises(ValueError, match="counter"):
        plan.run(counter=3, timeout_us=TIMEOUT_US)
    plan.free()
    _valid_plan_still_runs(queue, pol, e1, l1)


def test_library_refusals_before_anything_is_allocated(golden, queue):
    """rcbf_aql_closed_loop_plan called as aql.py calls it, one argument wrong at a time."""
    from rcbf_amd import _lib, aql
    pol = case(golden, "cars", 64)[5]
    (e1, l1), = _twins("cars", n=1)
    o = e1.make_outputs()
    a = e1._step_args(l1, o, True)
    u = torch.zeros(B, 1, device="cuda")
    traj = e1.make_trajectory(K, ("done", "term_obs"))

    def call(u_ptr=u.data_ptr(), flags=0, mask=0, pitch=0, term=None, n_o=pol.n_o, hidden=pol.hidden, mode=0,
             span=None, outs=None):
        h = ctypes.c_void_p()
        rc = _lib.load().rcbf_aql_closed_loop_plan(
            queue.handle, ctypes.byref(l1._prm), B, K, *[v or None for v in a[2:6]], u_ptr, None, None, 0,
            *[v or None for v in (outs or a[9:17])], *a[17:20], span, flags, mask, pitch, term, e1.obs.data_ptr(),
            pol.packed.data_ptr(), n_o, pol.n_u, hidden, mode, 0, None, 0, ctypes.byref(h))
        return rc, h

    span = torch.zeros(4 * 2 * K, dtype=torch.int64, device="cuda")
    bad = [({"flags": aql.PROFILE}, E_BAD_MODE), ({"flags": 8}, E_BAD_MODE), ({"span": span.data_ptr()}, E_BAD_MODE),
           ({"mode": 2}, E_BAD_MODE), ({"n_o": pol.n_o + 2}, E_BAD_SHAPE), ({"hidden": 48}, E_BAD_SHAPE),
           ({"u_ptr": e1.obs.data_ptr()}, E_BAD_SHAPE),                       # the action buffer inside obs
           ({"u_ptr": pol.packed.data_ptr() + 64}, E_BAD_SHAPE),              # ... inside the weights
           ({"u_ptr": u.data_ptr() + 2}, E_BAD_SHAPE),                        # misaligned
           ({"mask": aql.TRAJ_TERM_OBS, "pitch": 128}, E_BAD_MODE),           # the bit without the pointer
           ({"mask": aql.TRAJ_DONE, "pitch": 64}, E_BAD_SHAPE)]               # P < B
    for kw, want in bad:
        rc, h = call(**kw)
        assert rc == want and not h.value, (kw, rc)
    # the action buffer inside a recorded array's extent (its last row)
    outs = list(a[9:17])
    outs[4] = traj["done"].data_ptr()
    rc, h = call(u_ptr=traj["term_obs"]._base[K - 1].data_ptr(), mask=aql.TRAJ_DONE | aql.TRAJ_TERM_OBS, pitch=128,
                 term=traj["term_obs"].data_ptr(), outs=outs)
    assert rc == E_BAD_SHAPE and not h.value
    rc, h = call(flags=aql.PROFILE_ENDS)  # ... and a valid one
    assert rc == 0 and h.value and _lib.load().rcbf_aql_plan_dispatches(h) == 2 * K
    _lib.load().rcbf_aql_plan_free(h)


def test_profile_ends_times_the_whole_run(golden, queue):
    pol = case(golden, "cars", 64)[5]
    (e1, l1), = _twins("cars", n=1)
    from rcbf_amd import aql
    for steps in (1, 3):
        plan = queue.closed_loop_plan(e1, pol, l1, steps, evaluate=True, fence_flags=aql.PROFILE_ENDS)
        plan.run(timeout_us=TIMEOUT_US)
        t = plan.times_ns()
        assert t.shape == (steps, 2)
        assert 0 < t[0, 0] < t[0, 1] <= t[steps - 1, 1] and t[0, 0] <= t[steps - 1, 0]
        period = int(t[steps - 1, 1] - t[0, 0])
        assert 0 < period < 1_000_000_000
        plan.free()
