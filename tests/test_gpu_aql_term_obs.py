"""Trajectory plans that keep the terminal observation
(rcbf_aql_safe_step_term_plan, k_safe_steps_term; a "term_obs" field in
AqlQueue.safe_step_plan(trajectory=...)).

The oracle is that of test_gpu_aql_trajectory.py -- a twin env stepped by K
single env.safe_step launches, every recorded row torch.equal to the twin's
outputs after that step, the final state, env.obs and outputs dict equal to the
twin's -- plus a THIRD env for the terminal rows: before every twin step its
pre-step state is kept, and if the step sets done anywhere that state is loaded
into the third env, which takes the same action with auto_reset=False; its obs
row is the expected term_obs[j][i] of every env i with done set, bit for bit.
term_obs is sentinel-filled first and compared WHOLE against an array that
holds the sentinel everywhere else: steps without a reset, the columns [B, P)
and the rows >= K are never written."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_aql_fused import _assert_same, _pool, _snapshot, _twins, queue  # noqa: F401 (queue: the fixture)
from test_gpu_aql_trajectory import ALL, SENTINEL, _alloc, _check

pytestmark = pytest.mark.gpu

E_BAD_MODE, E_BAD_SHAPE = 1001, 1002
FIELDS = ALL + ("status", "term_obs")


def _envs(mode, B, hazards=3, **layer_kw):
    """Three identical (env, layer) pairs: the twin, the plan's env, the terminal-row env."""
    if mode == "SimulatedCars" or hazards <= 3:
        return _twins(mode, B, n=3, hazards=hazards, **layer_kw)
    import bench
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedUnicycleEnv
    from test_gpu_headline_parity import Args
    ang = np.linspace(0.0, 2.0 * np.pi, hazards, endpoint=False)
    locs = 1.6 * np.stack([np.cos(ang), np.sin(ang)], 1)
    out = []
    for _ in range(3):
        env = BatchedUnicycleEnv(B, device=torch.device("cuda", 0), seed=77, hazards_locations=locs)
        layer = CBFQPLayer(env, Args(), gamma_b=20.0)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        bench.init_states(env, gen, "Unicycle")
        out.append((env, layer))
    return out


def _load(envs, step=None, x=None, aux=None):
    for env, _ in envs:
        env.load_state(x=x, aux=aux, step=step)


def _twin_rows(e1, l1, e3, l3, pool, K, o1, o3, want_term, auto_reset=True, **kw):
    """K single launches of the twin; the outputs after every step, and in
    want_term[j, i] the terminal row of every env i that step j resets."""
    rows, resets = {}, 0
    for j in range(K):
        pre = (e1.x.clone(), e1.aux.clone(), e1.step_count.clone())
        u = pool[j % len(pool)]
        e1.safe_step(u, l1, outputs=o1, auto_reset=auto_reset, **kw)
        rows[j] = {"obs": e1.obs.clone(), **{f: o1[f].clone() for f in ("u", "reward", "cost", "done", "goal_met")}}
        idx = torch.nonzero(o1["done"]).flatten()
        if auto_reset and idx.numel():
            e3.x.copy_(pre[0])
            e3.aux.copy_(pre[1])
            e3.step_count.copy_(pre[2])
            e3.safe_step(u, l3, outputs=o3, auto_reset=False, **kw)
            assert torch.equal(o3["done"], o1["done"]) and torch.equal(o3["u"], o1["u"])
            want_term[j, idx] = e3.obs[idx]
            resets += int(idx.numel())
    return rows, resets


def _case(queue, envs, K, recorded=FIELDS, pool_n=7, dispatches=1, runs=1, auto_reset=True, step_kw=None):  # noqa: F811
    (e1, l1), (e2, l2), (e3, l3) = envs
    step_kw = step_kw or {}
    pool = _pool(e1, pool_n)
    o1, o2, o3 = e1.make_outputs(), e2.make_outputs(), e3.make_outputs()
    traj = _alloc(e2, K + 1, FIELDS)
    want_term = traj["term_obs"]._base.clone()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, trajectory={f: traj[f] for f in recorded},
                                auto_reset=auto_reset, **step_kw)
    assert plan.dispatches == dispatches
    total = 0
    for _ in range(runs):
        rows, resets = _twin_rows(e1, l1, e3, l3, pool, K, o1, o3, want_term, auto_reset, **step_kw)
        total += resets
        plan.run()
        torch.cuda.synchronize()
        _check(e2, {f: t for f, t in traj.items() if f != "term_obs"}, recorded, rows, K)
        assert torch.equal(traj["term_obs"]._base, want_term), "term_obs"
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()
    return traj, rows, total


def test_cars_resets_on_chosen_steps_in_chosen_lanes(queue):  # noqa: F811
    """B = 65 (a full wave and a one-lane wave), K = 6: resets on steps 0, 1
    and K - 1, on different steps in different lanes of the first wave, and in
    the second wave's only lane."""
    B, K = 65, 6
    envs = _envs("SimulatedCars", B)
    step = np.full(B, 10, np.int32)
    step[[0, 7]] = 299            # step 0
    step[[1, 63, 64]] = 298       # step 1
    step[[5, 33]] = 300 - K       # step K - 1
    step[20] = 297                # step 2
    _load(envs, step=step)
    traj, rows, resets = _case(queue, envs, K)
    assert resets == 8
    d = traj["done"][:K].cpu().numpy()
    assert d[0, [0, 7]].all() and d[1, [1, 63, 64]].all() and d[K - 1, [5, 33]].all() and d[2, 20] and d.sum() == 8


def test_cars_every_env_resets(queue):  # noqa: F811
    traj, rows, resets = _case(queue, _envs("SimulatedCars", 65), 310)
    assert resets >= 65 and bool(traj["done"][:310].any(0).all())  # the start steps differ: an env may end two


@pytest.mark.parametrize("hazards", [1, 5, 8])
def test_unicycle_resets_by_time_limit_and_by_goal(queue, hazards):  # noqa: F811
    """B = 130; some envs a few steps from the 1 000-step limit, some inside
    the goal's radius (0.3 around (2.5, 2.5)): goal_met fires on step 0 and
    ends the episode.  k = 5 with per-env sigma rows."""
    B, K = 130, 8
    envs = _envs("Unicycle", B, hazards=hazards)
    step = np.full(B, 3, np.int32)
    step[[0, 64, 129]] = 999
    step[[2, 70]] = 998
    step[[9]] = 1000 - K
    x = envs[0][0].state.cpu().numpy().copy()
    near = [4, 5, 66, 128]
    x[near] = np.array([2.5 - 0.25 * np.cos(0.3), 2.5 - 0.25 * np.sin(0.3), 0.3])  # 0.25 away; a step moves 0.022
    aux = np.sqrt(((2.5 - x[:, :2]) ** 2).sum(1))
    _load(envs, x=x, aux=aux, step=step)
    step_kw = {}
    if hazards == 5:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        step_kw = {"sigma": (0.2 * torch.rand(B, 3, device="cuda", generator=gen) + 0.05).contiguous()}
    traj, rows, resets = _case(queue, envs, K, step_kw=step_kw)
    d, g = traj["done"][:K].cpu().numpy(), traj["goal_met"][:K].cpu().numpy()
    assert d[0, [0, 64, 129]].all() and d[1, [2, 70]].all() and d[K - 1, 9]
    assert g[:, near].any(0).all() and (d[:, near] >= g[:, near]).all(), "the envs at the goal's edge met it"
    assert resets >= 10


def test_cars_column_priors(queue):  # noqa: F811
    B, K = 65, 4
    envs = _envs("SimulatedCars", B)
    step = np.full(B, 50, np.int32)
    step[[3, 64]] = 298
    _load(envs, step=step)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    nc = len(envs[0][0].PRIOR_COLS["SimulatedCars"])
    step_kw = {"sigma": (0.2 * torch.rand(nc, B, device="cuda", generator=gen) + 0.05).contiguous(),
               "prior_layout": "cols"}
    traj, rows, resets = _case(queue, envs, K, step_kw=step_kw)
    assert resets == 2


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_one_env_one_step_is_one_fused_dispatch(queue, mode):  # noqa: F811
    envs = _envs(mode, 1)
    _load(envs, step=np.array([299 if mode == "SimulatedCars" else 999], np.int32))
    traj, rows, resets = _case(queue, envs, 1, pool_n=1)
    assert resets == 1


@pytest.mark.parametrize("B", [32769, 65537])
def test_workgroup_sizes(queue, B):  # noqa: F811
    """The 128- and 256-thread kernels, each with a last wave of one live
    lane; every seventh env and the last one reset on step 1 or 2."""
    envs = _envs("SimulatedCars", B)
    step = np.full(B, 20, np.int32)
    step[::7] = 298
    step[3::7] = 297
    step[B - 1] = 298
    _load(envs, step=step)
    traj, rows, resets = _case(queue, envs, 3)
    assert resets == int((step >= 297).sum())


def test_two_chunks_with_a_reset_in_each(queue):  # noqa: F811
    """K = 4 097: step 4 096 is the second dispatch's only step; env 3 is
    loaded so that it resets there (103 + 4 097 = 14 x 300)."""
    B, K = 65, 4097
    envs = _envs("SimulatedCars", B)
    step = np.zeros(B, np.int32)
    step[3] = 103
    _load(envs, step=step)
    traj, rows, resets = _case(queue, envs, K, recorded=("u", "done", "term_obs"), pool_n=3, dispatches=2)
    d = traj["done"][:K]
    assert bool(d[4096, 3]) and bool(d[:4096].any()) and resets == int(d.sum())


def test_second_run_of_the_same_plan(queue):  # noqa: F811
    """The second run writes the rows of its own resets; what the first run
    wrote elsewhere stays (no element is cleared)."""
    B, K = 65, 5
    envs = _envs("SimulatedCars", B)
    step = np.full(B, 100, np.int32)
    step[[0, 64]] = 297     # run 1, step 2
    step[[10]] = 292        # run 2, step 2
    _load(envs, step=step)
    traj, rows, resets = _case(queue, envs, K, runs=2)
    assert resets == 3


def test_auto_reset_false_writes_nothing_to_term_obs(queue):  # noqa: F811
    B, K = 65, 4
    envs = _envs("SimulatedCars", B)
    step = np.full(B, 100, np.int32)
    step[[0, 64]] = 298
    _load(envs, step=step)
    traj, rows, resets = _case(queue, envs, K, auto_reset=False)
    assert resets == 0 and bool(traj["done"][:K].any())
    assert bool((traj["term_obs"]._base == SENTINEL[torch.float32]).all())


def _raw_term_plan(queue, env, layer, pool, K, o, ptrs, mask, pitch, term, flags=0):  # noqa: F811
    from rcbf_amd import _lib
    a = env._step_args(layer, o, True)
    outs = list(a[9:17])
    for j, f in enumerate(("obs", "u", "reward", "cost", "done", "goal_met", "status")):
        if f in ptrs:
            outs[j] = ptrs[f]
    arr = (ctypes.c_void_p * len(pool))(*[u.data_ptr() for u in pool])
    h = ctypes.c_void_p()
    rc = _lib.load().rcbf_aql_safe_step_term_plan(
        queue.handle, ctypes.byref(layer._prm), env.num_envs, K, *[v or None for v in a[2:6]], arr, len(pool), None,
        None, 0, *[v or None for v in outs], *a[17:20], None, flags, mask, pitch, term, ctypes.byref(h))
    return rc, h


def test_refusals(queue):  # noqa: F811
    from rcbf_amd import _lib, aql
    B, K = 65, 4
    (e1, l1), = _twins("SimulatedCars", B, n=1)
    pool = _pool(e1, 2)
    o = e1.make_outputs()
    traj = e1.make_trajectory(K, ALL + ("term_obs",))
    base = traj["term_obs"].data_ptr()
    assert base % 16 == 0
    T = aql.TRAJ_TERM_OBS
    raw = [(T, 128, None, 0, E_BAD_MODE),                       # the bit without the pointer
           (aql.TRAJ_DONE, 128, base, 0, E_BAD_MODE),           # the pointer without the bit
           (T, 128, base + 8, 0, E_BAD_SHAPE),                  # a misaligned base
           (T, 64, base, 0, E_BAD_SHAPE),                       # P < B
           (T, 128, base, aql.PER_STEP, E_BAD_MODE),            # no per-step form
           (T, 128, base, aql.PROFILE, E_BAD_MODE)]
    for mask, pitch, term, flags, want in raw:
        ptrs = {"done": traj["done"].data_ptr()} if mask & aql.TRAJ_DONE else {}
        rc, h = _raw_term_plan(queue, e1, l1, pool, K, o, ptrs, mask, pitch, term, flags)
        assert rc == want and not h.value, (mask, pitch, term, flags, rc)
    rc, h = _raw_term_plan(queue, e1, l1, pool, K, o, {}, T, 128, base, aql.PROFILE_ENDS)  # ... and a valid one
    assert rc == 0 and h.value and _lib.load().rcbf_aql_plan_dispatches(h) == 1
    _lib.load().rcbf_aql_plan_free(h)
    # an action buffer inside term_obs's (K, P, n_o) extent: the library, and the Python surface before it
    u_in = traj["term_obs"]._base[K - 1].reshape(-1)[:B].reshape(B, 1)
    assert u_in.is_contiguous()
    rc, h = _raw_term_plan(queue, e1, l1, [u_in], K, o, {}, T, 128, base)
    assert rc == E_BAD_MODE and not h.value
    with pytest.raises(ValueError, match="term_obs"):
        queue.safe_step_plan(e1, [u_in], l1, steps=K, outputs=o, trajectory=traj)
    for kw in ({"fused": False}, {"profile": True}):
        with pytest.raises(ValueError, match="fused"):
            queue.safe_step_plan(e1, pool, l1, steps=K, outputs=o, trajectory=traj, **kw)
    (e2, l2), = _twins("SimulatedCars", B, n=1, solver=_lib.SOLVER_PDIPM)
    with pytest.raises(ValueError, match="solver"):
        queue.safe_step_plan(e2, pool, l2, steps=K, outputs=e2.make_outputs(),
                             trajectory=e2.make_trajectory(K, ("done", "term_obs")))
    rc, h = _raw_term_plan(queue, e2, l2, pool, K, e2.make_outputs(), {}, T, 128, base)
    assert rc == E_BAD_MODE and not h.value


def test_terminal_observation_of_the_reference_episode(queue):  # noqa: F811
    """The reference's own 300-step cars episode (tests/golden/env_traj.npz),
    its recorded actions fed to a B = 1 plan.  The fixture's actions are the
    env's, not a safety layer's: the CBF layer alters 94 of the 300 (measured;
    the first at step 9, the action of step 299 passes unchanged), after which
    the plan's episode is no longer the reference's.  So the episode is
    teacher-forced in two parts.
    From the start, while the layer passes every action: obs[j] is the
    fixture's observation j + 1.  And the final step, from the fixture's state
    before it (loaded), where the layer passes the action again: a K = 1 plan
    that resets, whose term_obs row is the fixture's FINAL observation.  Both
    at test_gpu_parity.py's tolerance for this fixture (1e-12, relative), on
    top of the rows' rounding to fp32."""
    import os

    from test_abi_cpu import ROOT
    from test_gpu_headline_parity import _make
    d = np.load(os.path.join(ROOT, "tests", "golden", "env_traj.npz"))

    def err(got, want):
        want32 = want.astype(np.float32).astype(np.float64)
        return float(np.max(np.abs(got.double().cpu().numpy() - want32) / np.maximum(1.0, np.abs(want))))

    env, layer = _make("SimulatedCars", 1)
    env.reset(noise=d["cars_noise"][:1])
    assert np.array_equal(env.state_numpy(), d["cars_state"][:1, 0])
    acts = d["cars_actions"][0].reshape(300, 1, 1).astype(np.float32)
    us = [torch.tensor(a, device="cuda") for a in acts]
    traj = env.make_trajectory(300, ("obs", "u", "done", "term_obs"))
    traj["term_obs"]._base.fill_(SENTINEL[torch.float32])
    plan = queue.safe_step_plan(env, us, layer, outputs=env.make_outputs(), trajectory=traj)
    assert plan.dispatches == 1
    plan.run()
    torch.cuda.synchronize()
    same = traj["u"][:, 0, 0].cpu().numpy() == acts[:, 0, 0]
    n0 = int(np.argmin(same)) if not same.all() else 300
    print("actions the layer passed unchanged:", int(same.sum()), "of 300; the first altered one is step", n0)
    assert n0 >= 1 and same[299]
    e0 = err(traj["obs"][:n0, 0], d["cars_obs"][0, 1:n0 + 1])
    print("obs[:%d] against the fixture (as fp32): %.3g" % (n0, e0))
    assert e0 <= 1e-12
    assert bool(traj["done"][299, 0]) and not bool(traj["done"][:299].any())
    assert bool((traj["term_obs"][:299] == SENTINEL[torch.float32]).all())
    assert bool((traj["term_obs"][299] != SENTINEL[torch.float32]).all())
    plan.free()
    # the final step of the reference's episode
    env.load_state(x=d["cars_state"][:1, 299], aux=d["cars_t"][:1, 299], step=np.array([299], np.int32))
    traj = env.make_trajectory(1, ("obs", "u", "done", "term_obs"))
    plan = queue.safe_step_plan(env, us[299:], layer, outputs=env.make_outputs(), trajectory=traj)
    assert plan.dispatches == 1
    plan.run()
    torch.cuda.synchronize()
    assert bool(traj["done"][0, 0]) and traj["u"][0, 0, 0].item() == acts[299, 0, 0]
    e1 = err(traj["term_obs"][0, 0], d["cars_obs"][0, 300])
    print("term_obs of the final step against the fixture's final observation (as fp32): %.3g" % e1)
    assert e1 <= 1e-12
    assert env.step_count.item() == 0, "the env was reset"
    plan.free()
