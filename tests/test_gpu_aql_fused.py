"""The fused form of an AQL plan (csrc/rcbf_aql.hip, k_safe_steps in
csrc/rcbf_safe_step.hpp): ONE dispatch in which the lane that owns env i runs
all K steps of env i, against the same K steps launched one by one through
HIP (env.safe_step_seq).  Both forms run the same step body and every step
stores everything a step stores, so x, aux, step, episode, obs, u, reward,
cost, done and goal_met must be bit-identical afterwards -- across time-limit
resets, a u_RL pool whose length does not divide K, partial last waves at each
workgroup size, both envs and both prior layouts.  Plus: which form a plan
takes (plan.dispatches), and RCBF_AQL_PROFILE_ENDS on a one-packet plan."""
import pytest
import torch

import bench
from test_gpu_headline_parity import _make

pytestmark = pytest.mark.gpu


def _twins(mode, B, n=2, hazards=3, seed=77, **layer_kw):
    """n identical envs at the bench start states (as tests/test_gpu_aql.py)."""
    out = []
    for _ in range(n):
        env, layer = _make(mode, B, hazards=hazards, seed=seed)
        if layer_kw:
            from rcbf_amd.diff_cbf_qp import CBFQPLayer
            from test_gpu_headline_parity import Args
            layer = CBFQPLayer(env, Args(), gamma_b=20.0, **layer_kw)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(5)
        bench.init_states(env, gen, mode)
        out.append((env, layer))
    return out


def _snapshot(env, o):
    t = {"x": env.x, "aux": env.aux, "step": env.step_count, "episode": env.episode, "obs": env.obs}
    t.update({k: v for k, v in o.items() if v is not None})
    return {k: v.clone() for k, v in t.items()}


def _assert_same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _pool(env, n, seed=9):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    return [(torch.rand(env.num_envs, env.n_u, device="cuda", generator=gen) * 2 - 1).contiguous() for _ in range(n)]


@pytest.fixture(scope="module")
def queue():
    from rcbf_amd.aql import AqlQueue
    q = AqlQueue(torch.device("cuda", 0), profile=True)
    yield q
    q.close()


# 65: one full wave and a wave whose first lane is the only live one (64-thread workgroups); 1 000: a partial
# last wave, per-lane observation stores beside the staged ones; 32 769 and 65 537: the 128- and 256-thread
# workgroups (block_for_envs on a 256-CU device), each with a last wave of one live lane
@pytest.mark.parametrize("B", [65, 1000, 32769, 65537])
def test_fused_cars_plan_equals_hip_launches(queue, B):
    K = 310  # every env passes its 300-step time limit and resets; 310 is no multiple of the pool's 7
    (e1, l1), (e2, l2) = _twins("SimulatedCars", B)
    pool = _pool(e1, 7)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2)
    assert plan.dispatches == 1
    for _ in range(2):  # the second run continues from the first one's state like K more launches
        e1.safe_step_seq(pool, l1, outputs=o1, steps=K)
        plan.run()
        torch.cuda.synchronize()
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    assert int(e2.episode.min()) >= 1
    plan.free()


@pytest.mark.parametrize("hazards,B,K,layout", [(5, 1000, 1010, "cols"), (3, 65, 40, "rows")])
def test_fused_unicycle_plan_equals_hip_launches(queue, hazards, B, K, layout):
    """k = 5: past the 1 000-step limit, column priors with a per-env mean and
    sigma; k = 3: row priors."""
    (e1, l1), (e2, l2) = _twins("Unicycle", B, hazards=hazards)
    pool = _pool(e1, 7)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    shape = (len(e1.PRIOR_COLS["Unicycle"]), B) if layout == "cols" else (B, e1.n_s)
    sigma = (0.2 * torch.rand(*shape, device="cuda", generator=gen) + 0.05).contiguous()
    mean = (0.01 * torch.randn(*shape, device="cuda", generator=gen)).contiguous()
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    e1.safe_step_seq(pool, l1, mean=mean, sigma=sigma, outputs=o1, steps=K, prior_layout=layout)
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, mean=mean, sigma=sigma, outputs=o2, prior_layout=layout)
    assert plan.dispatches == 1
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    if K > 1000:
        assert int(e2.episode.min()) >= 1
    plan.free()


@pytest.mark.parametrize("hazards", [7, 8])
def test_fused_unicycle_many_hazards(queue, hazards):
    """k = 7 and 8: the kernels at the edge of the register file (k = 8 reads
    its parameter block with vector loads), in-kernel priors, B = 200 (three
    full waves and a partial one)."""
    import numpy as np
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedUnicycleEnv
    from test_gpu_headline_parity import Args
    B, K = 200, 60
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
    (e1, l1), (e2, l2) = pair
    pool = _pool(e1, 7)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    e1.safe_step_seq(pool, l1, outputs=o1, steps=K)
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2)
    assert plan.dispatches == 1
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()


def test_fused_false_builds_the_per_step_plan(queue):
    B, K = 1000, 20
    (e1, l1), (e2, l2), (e3, l3) = _twins("SimulatedCars", B, n=3)
    pool = _pool(e1, 7)
    o1, o2, o3 = e1.make_outputs(), e2.make_outputs(), e3.make_outputs()
    per_step = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, fused=False)
    fused = queue.safe_step_plan(e3, pool, l3, steps=K, outputs=o3)
    assert per_step.dispatches == K and fused.dispatches == 1
    e1.safe_step_seq(pool, l1, outputs=o1, steps=K)
    per_step.run()
    fused.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e2, o2), _snapshot(e3, o3))
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    per_step.free()
    fused.free()


def test_aliased_action_buffer_keeps_the_per_step_plan(queue):
    """A plan that reads its action from its own outputs["u"]: every step's
    action is the previous step's safe action, which only the per-step form
    (a dispatch boundary between the store and the load) gives."""
    B, K = 1000, 12
    (e1, l1), (e2, l2) = _twins("SimulatedCars", B)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    u0 = _pool(e1, 1)[0]
    o1["u"].copy_(u0)
    o2["u"].copy_(u0)
    plan = queue.safe_step_plan(e2, [o2["u"]], l2, steps=K, outputs=o2)
    assert plan.dispatches == K
    e1.safe_step_seq([o1["u"]], l1, outputs=o1, steps=K)
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    plan.free()


def test_profile_ends_on_one_packet_and_profile_per_step(queue):
    from rcbf_amd.aql import PROFILE_ENDS
    B = 1000
    (e1, l1), = _twins("SimulatedCars", B, n=1)
    pool = _pool(e1, 3)
    o1 = e1.make_outputs()
    # K = 1: one packet, first and last at once (it used to wait for a signal no packet carried)
    one = queue.safe_step_plan(e1, pool, l1, steps=1, outputs=o1, fence_flags=PROFILE_ENDS)
    assert one.dispatches == 1
    one.run(timeout_us=2_000_000)
    t = one.times_ns()
    assert t[0, 1] > t[0, 0] > 0
    one.free()
    # K = 20 fused: one packet, its start and end in rows 0 and K - 1, nothing between
    ends = queue.safe_step_plan(e1, pool, l1, steps=20, outputs=o1, fence_flags=PROFILE_ENDS)
    assert ends.dispatches == 1
    ends.run(timeout_us=2_000_000)
    t = ends.times_ns()
    assert 0 < t[0, 0] < t[0, 1] and tuple(t[19]) == tuple(t[0])
    assert (t[1:19] == 0).all()
    ends.free()
    # per-dispatch timestamps are per step by definition
    prof = queue.safe_step_plan(e1, pool, l1, steps=20, outputs=o1, profile=True)
    assert prof.dispatches == 20
    prof.free()
    e1.check_failures()


def test_other_solvers_keep_the_per_step_plan(queue):
    from rcbf_amd import _lib
    (e1, l1), = _twins("SimulatedCars", 256, n=1, solver=_lib.SOLVER_PDIPM)
    plan = queue.safe_step_plan(e1, _pool(e1, 3), l1, steps=3)
    assert plan.dispatches == 3
    plan.run()
    plan.free()
