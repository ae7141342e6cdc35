"""How the fused plan form's kernels (k_safe_steps, csrc/rcbf_safe_step.hpp)
walk the u_RL table: the address of step j + 2's buffer is fetched and step
j + 1's action loaded while step j runs.  Every case is bit-equal to the same
steps launched one by one through HIP (env.safe_step_seq) on a twin env:
plans cut into two dispatches (the second starts at a non-zero table index),
plans shorter than the look-ahead and pools of one buffer, a unicycle hazard
count from either side of the kernel's plain / accumulation-register split
(fused_plain in csrc/rcbf_safe_step.hpp: k = 1 and k = 2), and a pool buffer
that is only 4-byte aligned."""
import pytest
import torch

from test_gpu_aql_fused import _assert_same, _pool, _snapshot, _twins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def queue():
    from rcbf_amd.aql import AqlQueue
    q = AqlQueue(torch.device("cuda", 0))
    yield q
    q.close()


def _run_both(queue, twins, pool, K, dispatches=1, **kw):
    (e1, l1), (e2, l2) = twins
    o1, o2 = e1.make_outputs(), e2.make_outputs()
    e1.safe_step_seq(pool, l1, outputs=o1, steps=K, **kw)
    plan = queue.safe_step_plan(e2, pool, l2, steps=K, outputs=o2, **kw)
    assert plan.dispatches == dispatches
    plan.run()
    torch.cuda.synchronize()
    _assert_same(_snapshot(e1, o1), _snapshot(e2, o2))
    e1.check_failures()
    e2.check_failures()
    plan.free()
    return e2


def test_chunked_plan_continues_the_walk_in_its_second_dispatch(queue):
    """K = 4 096 + 5 steps are two dispatches; with a pool of 3 the second one
    starts at table index 4 096 % 3 = 1 and the index wraps over a thousand
    times.  B = 200: three full waves and a partial one.  Every env passes its
    300-step limit 13 times, so the register copy of the episode counter is
    stored and carried across both dispatches."""
    K = 4096 + 5
    twins = _twins("SimulatedCars", 200)
    e2 = _run_both(queue, twins, _pool(twins[0][0], 3), K, dispatches=2)
    assert int(e2.episode.min()) >= K // 300


@pytest.mark.parametrize("K,n_pool", [(2, 1), (3, 2)])
@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_short_plans_and_tiny_pools(queue, mode, K, n_pool):
    """K = 2 on one buffer: both steps read it, and nothing is loaded for a
    third step.  K = 3 on two.  B = 65: a full wave and a wave of one lane."""
    twins = _twins(mode, 65, hazards=3)
    _run_both(queue, twins, _pool(twins[0][0], n_pool), K)


@pytest.mark.parametrize("hazards", [1, 2])
def test_unicycle_on_either_side_of_the_plain_split(queue, hazards):
    """k = 1 keeps the loop's values in plain variables, k = 2 in accumulation
    registers with the table walked through readfirstlane.  Column priors."""
    B, K = 200, 60
    twins = _twins("Unicycle", B, hazards=hazards)
    e1 = twins[0][0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    shape = (len(e1.PRIOR_COLS["Unicycle"]), B)
    sigma = (0.2 * torch.rand(*shape, device="cuda", generator=gen) + 0.05).contiguous()
    mean = (0.01 * torch.randn(*shape, device="cuda", generator=gen)).contiguous()
    _run_both(queue, twins, _pool(e1, 7), K, mean=mean, sigma=sigma, prior_layout="cols")


def test_pool_buffer_at_a_four_byte_offset(queue):
    """The action's load assumes no more than a float's alignment: the second
    of three buffers is a view one float into a larger allocation."""
    B, K = 65, 10
    twins = _twins("SimulatedCars", B)
    e1 = twins[0][0]
    pool = _pool(e1, 3)
    big = torch.empty(B * e1.n_u + 8, device="cuda", dtype=torch.float32)
    odd = big[1:1 + B * e1.n_u].view(B, e1.n_u)
    odd.copy_(pool[1])
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    pool[1] = odd
    _run_both(queue, twins, pool, K)
