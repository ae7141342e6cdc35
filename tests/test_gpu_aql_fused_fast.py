"""The cars fused plan's straight-line loop (rcbf::k_safe_steps_fast,
csrc/rcbf_safe_steps_fast.hpp), which the plan builder dispatches in
k_safe_steps's place when every wave is full.  Every case is bit-equal
(torch.equal on x, aux, step, episode, obs, u, reward, cost, done) to a twin
env stepped by K single `env.safe_step` launches -- the per-step kernel, which
shares no loop with the code under test -- and `plan.form` says that the kernel
meant really ran: odd and even step counts on pools shorter than the two-ahead
walk, resets on either half of an iteration, the hand-over to the library sine
in the middle of a plan, the plans that keep k_safe_steps, and the shapes the
other fused tests run."""
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


def _launches(env, layer, pool, K, o, **kw):
    for j in range(K):
        env.safe_step(pool[j % len(pool)], layer, outputs=o, **kw)


def _check(queue, e1, l1, e2, l2, K, pool, form="fused_fast", runs=1, dispatches=1, plan_kw=None, **kw):
    """K steps `runs` times over: K launches on e1, one plan on e2, compared after every run."""
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, **kw, **(plan_kw or {}))
    assert plan.form == form
    assert plan.dispatches == dispatches
    for _ in range(runs):
        _launches(e1, l1, pool, K, o1, **kw)
        plan.run()
        torch.cuda.synchronize()
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()
    return o1, o2


@pytest.mark.parametrize("B", [64, 128, 320])
@pytest.mark.parametrize("K", [2, 3, 4, 7])
def test_short_plans_on_short_pools(queue, B, K):
    """Odd and even step counts (the odd last step runs in the second loop), on pools of 1, 2 and 3 buffers:
    the walk asks for the actions of steps j + 2 and j + 3 and wraps the pool more than once per iteration."""
    (e1, l1), (e2, l2) = _twins(CARS, B)
    for n_pool in (1, 2, 3):
        _check(queue, e1, l1, e2, l2, K, _pool(e1, n_pool, seed=9 + n_pool))


def test_resets_on_either_half_of_an_iteration(queue):
    """Step counters per group of 16 lanes: the groups reset on the plan's first step (the first half of an
    iteration), its second (the second half; with the group before it, both halves of one iteration in one wave),
    third, fourth, fifth and sixth and last step, or never."""
    B, K = 128, 6
    (e1, l1), (e2, l2) = _twins(CARS, B)
    st = torch.tensor([299, 298, 297, 296, 295, 294, 0, 150], dtype=torch.int32, device="cuda").repeat_interleave(16)
    for e in (e1, e2):
        e.load_state(step=st)
    ep0 = e2.episode.clone()
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 5))
    assert torch.equal(e2.step_count, torch.where(st >= 294, st + K - 300, st + K).to(torch.int32))
    assert torch.equal((e2.episode - ep0).to(torch.int32), (st >= 294).to(torch.int32))


def test_every_env_resets_in_one_plan(queue):
    B, K = 64, 301
    (e1, l1), (e2, l2) = _twins(CARS, B)
    st = (torch.arange(B, device="cuda", dtype=torch.int32) * 37) % 300  # staggered: a reset in most iterations
    for e in (e1, e2):
        e.load_state(step=st)
    ep0 = e2.episode.clone()
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 7))
    assert int((e2.episode - ep0).min()) >= 1


@pytest.mark.parametrize("t0,first_out", [(6.43, 4), (6.45, 3)])
def test_hand_over_to_the_library_sine(queue, t0, first_out):
    """auto_reset = 0 and t loaded so that 0.2 t passes 1.3 at step `first_out` of an 8-step plan (counted from
    0: an even step is an iteration's first half, an odd one its second).  In wave 0 half of the lanes cross and
    the others stay far inside the range (they get the series' bits in the second loop too); wave 1 never
    crosses and stays in the first loop.  Every step's stores are there: the final state and the last step's
    outputs equal the launches'."""
    B, K = 128, 8
    (e1, l1), (e2, l2) = _twins(CARS, B)
    aux = torch.full((B,), 1.0, dtype=torch.float64, device="cuda")
    aux[:32] = t0
    assert 0.2 * (t0 + 0.02 * (first_out - 1)) <= 1.3 < 0.2 * (t0 + 0.02 * first_out)
    for e in (e1, e2):
        e.load_state(aux=aux, step=torch.full((B,), 10, dtype=torch.int32))
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 3), auto_reset=False)
    assert torch.equal(e2.aux[:32], e1.aux[:32]) and float(e2.aux[0]) > 6.5


@pytest.mark.parametrize("B", [65, 100])
def test_partial_wave_keeps_the_fused_loop(queue, B):
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _check(queue, e1, l1, e2, l2, 6, _pool(e1, 3), form="fused")


def test_status_output_keeps_the_fused_loop(queue):
    """The fast kernels are built for a null status_out (what BatchedEnv passes): a plan given one takes
    k_safe_steps, which writes it.  The pointer goes in through the env's cached argument list."""
    B, K = 128, 4
    (e1, l1), (e2, l2) = _twins(CARS, B)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    args = e2._step_args(l2, o2, True)
    assert args[15] == 0
    args[15] = status.data_ptr()
    try:
        plan = queue.safe_step_plan(e2, _pool(e2, 3), l2, steps=K, outputs=o2)
    finally:
        args[15] = 0
    assert plan.form == "fused"
    _launches(e1, l1, _pool(e1, 3), K, o1)
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    assert int(status.abs().max()) == 0
    plan.free()


def test_trajectory_plan_and_forced_plans_keep_their_kernels(queue):
    B, K = 128, 5
    (e1, l1), (e2, l2) = _twins(CARS, B)
    pool = _pool(e1, 3)
    _check(queue, e1, l1, e2, l2, K, pool, form="fused", plan_kw={"fast": False})
    _check(queue, e1, l1, e2, l2, K, pool, form="per_step", dispatches=K, plan_kw={"fused": False})
    _check(queue, e1, l1, e2, l2, 1, pool, form="per_step")
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, trajectory=True)
    assert plan.form == "fused"
    _launches(e1, l1, pool, K, o1)
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    plan.free()


@pytest.mark.parametrize("layout", ["cols", "rows"])
def test_per_env_sigma(queue, layout):
    B = 192
    (e1, l1), (e2, l2) = _twins(CARS, B)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    shape = (len(e1.PRIOR_COLS[CARS]), B) if layout == "cols" else (B, e1.n_s)
    sigma = (0.5 * torch.rand(*shape, device="cuda", generator=gen) + 0.05).contiguous()
    st = torch.tensor([297, 298, 299, 0], dtype=torch.int32, device="cuda").repeat_interleave(48)
    for e in (e1, e2):
        e.load_state(step=st)
    _check(queue, e1, l1, e2, l2, 6, _pool(e1, 4), sigma=sigma, prior_layout=layout)


def test_plan_run_twice_and_state_loaded_between_runs(queue):
    B, K = 128, 5
    (e1, l1), (e2, l2), (e3, l3) = _twins(CARS, B, n=3)
    pool = _pool(e1, 3)
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2)
    assert plan.form == "fused_fast"
    for r in range(3):
        if r == 2:
            # fresh states (the third twin's start state, one step on) and step counts that reset inside the run
            e3.safe_step(pool[0], l3)
            torch.cuda.synchronize()
            st = torch.tensor([297, 298, 299, 0], dtype=torch.int32, device="cuda").repeat_interleave(32)
            for e in (e1, e2):
                e.load_state(x=e3.state, aux=e3.aux, step=st)
        _launches(e1, l1, pool, K, o1)
        plan.run()
        torch.cuda.synchronize()
        _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e2.check_failures()
    plan.free()


def test_two_dispatches(queue):
    """4 097 steps are two chunks: 4 096 in the first loop, and one step, which the second loop runs."""
    B, K = 64, 4096 + 1
    (e1, l1), (e2, l2) = _twins(CARS, B)
    _check(queue, e1, l1, e2, l2, K, _pool(e1, 7), dispatches=2)


def test_code_object_without_the_fast_kernels_plans_as_before(tmp_path):
    """A queue opened on a copy of librcbf_steps.co with no _fast.co beside it builds the same plan on k_safe_steps."""
    import os
    import shutil

    from rcbf_amd import _lib
    from rcbf_amd.aql import AqlQueue
    co = str(tmp_path / "steps.co")
    shutil.copy(os.path.join(os.path.dirname(_lib.LIB_PATH), "librcbf_steps.co"), co)
    q = AqlQueue(torch.device("cuda", 0), code_object=co)
    try:
        (e1, l1), (e2, l2) = _twins(CARS, 128)
        _check(q, e1, l1, e2, l2, 4, _pool(e1, 3), form="fused")
    finally:
        q.close()
