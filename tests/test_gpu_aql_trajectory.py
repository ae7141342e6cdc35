"""Trajectory plans (rcbf_aql_safe_step_traj_plan, k_safe_steps_traj;
AqlQueue.safe_step_plan(trajectory=...)): a K-step AQL plan that keeps EVERY
step's outputs, step j in row j of each recorded field's (K, P, w) array.

The oracle in every case is a twin env stepped by K single env.safe_step
launches, its outputs cloned after each: the trajectory's rows must be
torch.equal to those clones (the reset observation on a step that resets
included), and afterwards x, aux, step, episode, env.obs and the outputs dict
must equal the twin's.  Trajectories are allocated with one extra row and
filled with a sentinel first: rows >= K, the columns [B, P) and the fields that
are not recorded must still hold it."""
import ctypes

import pytest
import torch

from test_gpu_aql_fused import _assert_same, _pool, _snapshot, _twins, queue  # noqa: F401 (queue: the fixture)

pytestmark = pytest.mark.gpu

ALL = ("obs", "u", "reward", "cost", "done", "goal_met")
SENTINEL = {torch.float32: -12345.5, torch.uint8: 0xA5, torch.int32: -77}
E_BAD_MODE, E_BAD_SHAPE = 1001, 1002


def _alloc(env, rows, fields=ALL + ("status",)):
    """env.make_trajectory(rows, fields), every element of every array (the
    padding columns too) set to its dtype's sentinel."""
    t = env.make_trajectory(rows, fields)
    for v in t.values():
        v._base.fill_(SENTINEL[v.dtype])
    return t


def _twin_rows(env, layer, pool, K, o, keep=None, **kw):
    """K single launches; {j: the outputs after step j} for j in keep (None: all)."""
    rows = {}
    for j in range(K):
        env.safe_step(pool[j % len(pool)], layer, outputs=o, **kw)
        if keep is None or j in keep:
            rows[j] = {"obs": env.obs.clone(), **{f: o[f].clone() for f in ("u", "reward", "cost", "done", "goal_met")}}
    return rows


def _check(env, traj, recorded, rows, K):
    """traj: everything allocated (the recorded fields and the others)."""
    B = env.num_envs
    cars = env.dynamics_mode == "SimulatedCars"
    for f, t in traj.items():
        base, sent = t._base, SENTINEL[t.dtype]
        written = f in recorded and not (f == "goal_met" and cars)
        if not written:
            assert bool((base == sent).all()), f"{f}: not recorded, but written"
            continue
        assert bool((base[K:] == sent).all()), f"{f}: a row >= K was written"
        assert bool((base[:, B:] == sent).all()), f"{f}: a column >= B was written"
        if f == "status":
            assert bool((t[:K] == 0).all()), "status"  # RCBF_QP_OK: the twin has no status output, its fail_flag is clear
            continue
        for j, r in rows.items():
            assert torch.equal(t[j], r[f]), (f, j)


def _case(queue, pair, K, recorded, pool_n=7, dispatches=1, keep=None, step_kw=None, alloc=ALL + ("status",),
          **plan_kw):
    (e1, l1), (e2, l2) = pair
    step_kw = step_kw or {}
    pool = _pool(e1, pool_n)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    traj = _alloc(e2, K + 1, alloc)
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, trajectory={f: traj[f] for f in recorded},
                                **step_kw, **plan_kw)
    assert plan.dispatches == dispatches
    assert set(plan.trajectory) == set(recorded)
    rows = _twin_rows(e1, l1, pool, K, o1, keep, **step_kw)
    plan.run()
    torch.cuda.synchronize()
    _check(e2, traj, recorded, rows, K)
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()
    return traj, rows


def test_cars_trajectory_with_resets_inside_the_plan(queue):
    """B = 65: a full wave and a one-lane wave (P = 128); K = 310: every env
    passes its 300-step limit, so rows with done and the reset observation are
    compared.  All fields and the status; the cars goal_met is not recorded."""
    traj, rows = _case(queue, _twins("SimulatedCars", 65), 310, ALL + ("status",))
    assert traj["obs"].stride(0) == 128 * 10
    done_rows = [j for j, r in rows.items() if bool(r["done"].any())]
    assert done_rows and bool(traj["done"][:310].any(0).all())


def _unicycle_pair(hazards, B):
    if hazards <= 3:
        return _twins("Unicycle", B, hazards=hazards)
    import numpy as np

    import bench
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedUnicycleEnv
    from test_gpu_headline_parity import Args
    ang = np.linspace(0.0, 2.0 * np.pi, hazards, endpoint=False)
    locs = 1.6 * np.stack([np.cos(ang), np.sin(ang)], 1)
    pair = []
    for _ in range(2):
        env = BatchedUnicycleEnv(B, device=torch.device("cuda", 0), seed=77, hazards_locations=locs)
        layer = CBFQPLayer(env, Args(), gamma_b=20.0)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        bench.init_states(env, gen, "Unicycle")
        pair.append((env, layer))
    return pair


@pytest.mark.parametrize("hazards", [1, 2, 8])
def test_unicycle_trajectory(queue, hazards):
    """k = 1, 2 and 8 (the parameters and the row strides from LDS); B = 200:
    three full waves and a partial one; k = 2 with column priors."""
    B, K = 200, 60
    pair = _unicycle_pair(hazards, B)
    step_kw = {}
    if hazards == 2:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(11)
        shape = (len(pair[0][0].PRIOR_COLS["Unicycle"]), B)
        step_kw = {"sigma": (0.2 * torch.rand(*shape, device="cuda", generator=gen) + 0.05).contiguous(),
                   "mean": (0.01 * torch.randn(*shape, device="cuda", generator=gen)).contiguous(),
                   "prior_layout": "cols"}
    _case(queue, pair, K, ALL, step_kw=step_kw)


@pytest.mark.parametrize("recorded", [("reward", "done"), ("obs",)])
def test_masks_record_only_the_chosen_fields(queue, recorded):
    """The other outputs are overwritten in place and end as the twin's
    last-step values (the outputs dict and env.obs, compared by _case)."""
    _case(queue, _twins("Unicycle", 200, hazards=3), 25, recorded)


def test_cars_goal_met_and_a_null_status_are_not_written_through(queue):
    """goal_met is in the dict, but never recorded for the cars env; no status
    array is passed at all (a null pointer, which must not be advanced)."""
    _case(queue, _twins("SimulatedCars", 200), 20, ("done", "goal_met"))


@pytest.mark.parametrize("B", [32769, 65537])
def test_workgroup_sizes(queue, B):
    """The 128- and 256-thread kernels, each with a last wave of one live lane."""
    _case(queue, _twins("SimulatedCars", B), 3, ALL)


def test_two_chunks(queue):
    K = 4096 + 5
    traj, rows = _case(queue, _twins("SimulatedCars", 65), K, ("u", "reward", "done"), pool_n=3, dispatches=2)
    assert set(rows) >= {4094, 4095, 4096, 4097, K - 1}


@pytest.mark.parametrize("how", ["fused_false", "profile", "one_step", "pdipm"])
def test_per_step_form(queue, how):
    from rcbf_amd import _lib
    K = 1 if how == "one_step" else 12
    kw = {"fused_false": {"fused": False}, "profile": {"profile": True}}.get(how, {})
    pair = _twins("SimulatedCars", 200, **({"solver": _lib.SOLVER_PDIPM} if how == "pdipm" else {}))
    _case(queue, pair, K, ALL, dispatches=K, **kw)


def test_second_run_rewrites_the_rows_from_the_state_the_first_left(queue):
    B, K = 200, 30
    (e1, l1), (e2, l2) = _twins("SimulatedCars", B)
    pool = _pool(e1, 7)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, trajectory=True)
    assert plan.dispatches == 1 and set(plan.trajectory) == set(ALL)
    for _ in range(2):
        rows = _twin_rows(e1, l1, pool, K, o1)
        plan.run()
        torch.cuda.synchronize()
        for f in ("obs", "u", "reward", "cost", "done"):
            assert plan.trajectory[f].shape[:2] == (K, B)
            for j in range(K):
                assert torch.equal(plan.trajectory[f][j], rows[j][f]), (f, j)
        assert not bool(plan.trajectory["goal_met"].any())
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    plan.free()


def test_offsets_past_2_to_31_elements(queue):
    """Cars, obs only, B = 32 769 (P = 32 832), K = 6 600: K P 10 floats, 8.7
    GB in two chunks; row 6 541 is the first whose element offset (j P 10)
    exceeds 2^31."""
    B, K = 32769, 6600
    free = torch.cuda.mem_get_info()[0]
    if free < 24 * 2**30:
        pytest.skip(f"needs 24 GB of free device memory for an 8.7 GB trajectory, {free / 2**30:.1f} GB are free")
    P = (B + 63) // 64 * 64
    first = next(j for j in range(K) if j * P * 10 > 2**31)
    assert first == 6541
    keep = {0, 4095, 4096, first, K - 1}
    traj, rows = _case(queue, _twins("SimulatedCars", B), K, ("obs",), pool_n=3, dispatches=2, keep=keep,
                       alloc=("obs", "done"))
    assert set(rows) == keep
    del traj


def _raw_plan(queue, env, layer, pool, K, o, ptrs, mask, pitch, span=None):
    """rcbf_aql_safe_step_traj_plan called as aql.py calls it, with the output
    pointers, mask and pitch given; returns (rc, handle)."""
    from rcbf_amd import _lib
    a = env._step_args(layer, o, True)
    outs = list(a[9:17])
    for j, f in enumerate(("obs", "u", "reward", "cost", "done", "goal_met", "status")):
        if f in ptrs:
            outs[j] = ptrs[f]
    arr = (ctypes.c_void_p * len(pool))(*[u.data_ptr() for u in pool])
    h = ctypes.c_void_p()
    rc = _lib.load().rcbf_aql_safe_step_traj_plan(
        queue.handle, ctypes.byref(layer._prm), env.num_envs, K, *[v or None for v in a[2:6]], arr, len(pool), None,
        None, 0, *[v or None for v in outs], *a[17:20], None if span is None else span.data_ptr(), 0, mask, pitch,
        ctypes.byref(h))
    return rc, h


def test_rejections(queue):
    from rcbf_amd import _lib, aql
    B, K = 65, 4
    (e1, l1), = _twins("SimulatedCars", B, n=1)
    pool = _pool(e1, 2)
    o = e1.make_outputs()
    big = torch.empty(K * 256 * 10 + 16, dtype=torch.float32, device="cuda")
    base = big.data_ptr()
    assert base % 16 == 0
    cases = [({"obs": base}, aql.TRAJ_OBS, 66, None, E_BAD_SHAPE),        # P % 4 != 0
             ({"reward": base}, aql.TRAJ_REWARD, 64, None, E_BAD_SHAPE),  # P < B
             ({"obs": base + 4}, aql.TRAJ_OBS, 128, None, E_BAD_SHAPE),   # a 4-byte-offset observation base
             ({"obs": base + 8}, aql.TRAJ_OBS, 128, None, E_BAD_SHAPE),   # 8-byte: fine for a plain plan, not here
             ({"reward": base}, aql.TRAJ_REWARD, 128,
              torch.zeros(4 * 2 * K, dtype=torch.int64, device="cuda"), E_BAD_MODE)]  # span and a mask
    for ptrs, mask, pitch, span, want in cases:
        rc, h = _raw_plan(queue, e1, l1, pool, K, o, ptrs, mask, pitch, span)
        assert rc == want and not h.value, (ptrs, mask, pitch, rc)
    # the same call with a valid pitch and base builds a plan; mask 0 ignores the pitch
    for ptrs, mask, pitch in [({"obs": base}, aql.TRAJ_OBS, 128), ({}, 0, 3)]:
        rc, h = _raw_plan(queue, e1, l1, pool, K, o, ptrs, mask, pitch)
        assert rc == 0 and h.value
        assert _lib.load().rcbf_aql_plan_dispatches(h) == 1
        _lib.load().rcbf_aql_plan_free(h)
    # wrongly shaped / typed / strided trajectory dicts
    good = e1.make_trajectory(K)
    bad = [{"reward": torch.empty(K, B + 1, device="cuda")},                      # another B
           {"reward": torch.empty(K - 1, 128, device="cuda")[:, :B]},             # fewer rows than steps
           {"obs": torch.empty(K, 128, 10, device="cuda", dtype=torch.float64)[:, :B]},  # dtype
           {"obs": torch.empty(K, 128, 12, device="cuda")[:, :B, :10]},           # not dense in w
           {"reward": good["reward"], "cost": torch.empty(K, 192, device="cuda")[:, :B]},  # two pitches
           {"reward": torch.empty(K, 128)[:, :B]},                                 # host memory
           {"rewards": good["reward"]}]                                            # unknown field
    for t in bad:
        with pytest.raises(ValueError):
            queue.safe_step_plan(e1, pool, l1, steps=K, outputs=o, trajectory=t)
    with pytest.raises(ValueError):
        queue.safe_step_plan(e1, pool, l1, steps=K, outputs=o, trajectory=good,
                             span=torch.zeros(4 * 2 * K, dtype=torch.int64, device="cuda"))


def test_action_buffer_inside_a_recorded_array_keeps_the_per_step_plan(queue):
    """u_RL is row K - 1 of the recorded u array: inside the (K, P, n_u) extent
    the steps write (though not inside one step's (B, n_u)), so the plan takes
    the per-step form, where each step loads its action before it stores."""
    B, K = 65, 6
    (e1, l1), (e2, l2) = _twins("SimulatedCars", B)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    traj = _alloc(e2, K + 1)
    u0 = _pool(e1, 1)[0]
    u_in = traj["u"][K - 1]
    assert u_in.is_contiguous()
    u_in.copy_(u0)
    plan = queue.safe_step_plan(e2, [u_in], l2, steps=K, outputs=o2, trajectory={"u": traj["u"], "reward": traj["reward"]})
    assert plan.dispatches == K
    rows = _twin_rows(e1, l1, [u0], K, o1)
    plan.run()
    torch.cuda.synchronize()
    _check(e2, traj, ("u", "reward"), rows, K)
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    plan.free()
