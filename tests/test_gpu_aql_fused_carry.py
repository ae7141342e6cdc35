"""What the cars fused loop carries from one step into the next (fused_carry,
csrc/rcbf_safe_step.hpp): the fp32 observation row a step's tail stores is the
row the next step's layer reads, and the next step's rows are built from it in
that tail, from the next action.  Every case is bit-equal (torch.equal on x,
aux, step, episode, obs, u, reward, cost, done) to the same steps launched one
by one through HIP (env.safe_step_seq) on a twin env, whose kernel carries
nothing: resets on chosen steps, partial waves and an unaligned observation
buffer (the per-lane observation path), short plans and short pools (the action
the prebuilt rows use), plans of two dispatches, a plan run twice, a state
loaded between two runs (the prologue starts from HBM alone), per-env sigma in
both layouts, and the trajectory plan's rows."""
import pytest
import torch

from test_gpu_aql_fused import _assert_same, _pool, _snapshot, _twins

pytestmark = pytest.mark.gpu
CARS = "SimulatedCars"


@pytest.fixture(scope="module")
def queue():
    from rcbf_amd.aql import AqlQueue
    q = AqlQueue(torch.device("cuda", 0))
    yield q
    q.close()


def _check(queue, e1, l1, e2, l2, K, pool, runs=1, dispatches=1, **prior):
    """K steps `runs` times over: launches on e1, one plan on e2, compared after every run."""
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, **prior)
    assert plan.dispatches == dispatches
    for _ in range(runs):
        e1.safe_step_seq(pool, l1, outputs=o1, steps=K, **prior)
        plan.run()
        torch.cuda.synchronize()
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()
    return o1, o2


def _set_steps(envs, B):
    """Episode steps 297, 298, 299 and 0, one value per group of 32 lanes, so that each wave holds two of
    them: with the 300-step limit the groups reset on the plan's third, second and first step, or never."""
    st = torch.tensor([297, 298, 299, 0], dtype=torch.int32, device="cuda").repeat_interleave(32).repeat(B // 128)
    st = torch.cat([st, st.new_zeros(envs[0].num_envs - B)])  # envs past B start at 0 and never reset
    for e in envs:
        e.load_state(step=st)
    return st


def test_reset_on_chosen_steps(queue):
    B, K = 128, 5
    (e1, l1), (e2, l2) = _twins(CARS, B)
    st = _set_steps((e1, e2), B)
    ep0 = e2.episode.clone()
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 7))
    # the resets happened where they were planned, and the steps after them ran inside the plan
    want = torch.where(st == 0, K, st + K - 300).to(torch.int32)
    assert torch.equal(e2.step_count, want)
    assert torch.equal((e2.episode - ep0).to(torch.int32), (st != 0).to(torch.int32))


@pytest.mark.parametrize("B", [65, 100])
def test_partial_wave_takes_the_per_lane_observation_path(queue, B):
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _check(queue, e1, l1, e2, l2, 12, _pool(e1, 5))


def test_unaligned_observation_buffer(queue):
    """An observation buffer that is not 16-byte aligned: full waves take the per-lane path too.  A plan
    stores the rows in 8-byte halves, so its builder refuses a base that is only 4-byte aligned (checked
    here); the view 8 bytes into an aligned buffer is the unaligned buffer a plan can be given."""
    B = 128
    (e1, l1), (e2, l2) = _twins(CARS, B)
    buf = torch.zeros(B * e2.n_o + 1, dtype=torch.float32, device="cuda")
    e2.obs = buf[1:].view(B, e2.n_o)
    assert e2.obs.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="RCBF_E_BAD_SHAPE"):
        queue.safe_step_plan(e2, _pool(e2, 1), l2, steps=2, outputs=e2.make_outputs())
    for e in (e1, e2):
        e.obs = torch.zeros((B + 1) * e.n_o, dtype=torch.float32, device="cuda")[2:2 + B * e.n_o].view(B, e.n_o)
        assert e.obs.data_ptr() % 16 == 8
    _set_steps((e1, e2), B)
    _check(queue, e1, l1, e2, l2, 6, _pool(e1, 5))


@pytest.mark.parametrize("K,n_pool", [(2, 1), (3, 2), (1, 1)])
def test_short_plans_and_short_pools(queue, K, n_pool):
    B = 128
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _check(queue, e1, l1, e2, l2, K, _pool(e1, n_pool), runs=2)


def test_two_dispatches(queue):
    B, K = 128, 4096 + 3
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 7), dispatches=2)


def test_plan_run_twice_and_state_loaded_between_runs(queue):
    B, K = 128, 5
    (e1, l1), (e2, l2), (e3, l3) = _twins(CARS, B, n=3)
    pool = _pool(e1, 3)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2)
    for r in range(3):
        if r == 2:
            # fresh states (the third twin's start state, one step on) and step counts that reset inside the run
            e3.safe_step_seq(pool, l3, steps=1)
            torch.cuda.synchronize()
            for e in (e1, e2):
                e.load_state(x=e3.state, aux=e3.aux)
            _set_steps((e1, e2), B)
        e1.safe_step_seq(pool, l1, outputs=o1, steps=K)
        plan.run()
        torch.cuda.synchronize()
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e2.check_failures()
    plan.free()


@pytest.mark.parametrize("layout", ["cols", "rows"])
def test_per_env_sigma(queue, layout):
    B = 192
    (e1, l1), (e2, l2) = _twins(CARS, B)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    shape = (len(e1.PRIOR_COLS[CARS]), B) if layout == "cols" else (B, e1.n_s)
    sigma = (0.5 * torch.rand(*shape, device="cuda", generator=gen) + 0.05).contiguous()
    _set_steps((e1, e2), 128)  # the first two waves; the third never resets
    _check(queue, e1, l1, e2, l2, 6, _pool(e1, 4), sigma=sigma, prior_layout=layout)


def test_trajectory_rows_equal_launches(queue):
    B, K = 128, 7
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _set_steps((e1, e2), B)
    pool = _pool(e1, 3)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    fields = ("obs", "u", "reward", "cost", "done", "status")
    traj = e2.make_trajectory(K, fields=fields)
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, trajectory=traj)
    assert plan.dispatches == 1
    plan.run()
    torch.cuda.synchronize()
    for j in range(K):
        e1.safe_step_seq([pool[j % len(pool)]], l1, outputs=o1, steps=1)
        torch.cuda.synchronize()
        assert torch.equal(traj["obs"][j], e1.obs), j
        for f in ("u", "reward", "cost", "done"):
            assert torch.equal(traj[f][j], o1[f]), (f, j)
        assert int(traj["status"][j].abs().max()) == 0, j
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e2.check_failures()
    plan.free()
