"""ReplayMemory.push_trajectory (rcbf_traj_pack_replay_f64, k_traj_pack_replay):
the K x B transitions of a trajectory plan written straight into the replay
ring.

The oracle is a twin ReplayMemory filled by batch_push from arrays assembled
with torch from the same trajectory, following the field rules of
include/rcbf_hip.h literally; the two rings must then be equal BIT FOR BIT
(compared as int64) over every slot -- both start sentinel-filled, so slots that
must stay untouched are compared too -- and position and len() must be equal.
Most trajectories here are synthetic tensors (random fp32, random done, random
step0): the kernel does not care where they come from."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = {"SimulatedCars": (10, 1, 300, 0.02), "Unicycle": (7, 2, 1000, 0.02)}
SENT = -4321.25


class _Env:
    """What push_trajectory reads of an env."""

    def __init__(self, mode, B):
        self.dynamics_mode, self.num_envs = mode, B
        self.n_o, self.n_u, self.max_episode_steps, self.dt = DIMS[mode]

    def _trajectory_spec(self):
        return {"obs": (self.n_o, torch.float32), "u": (self.n_u, torch.float32), "reward": (0, torch.float32),
                "done": (0, torch.uint8), "term_obs": (self.n_o, torch.float32)}


def _synthetic(env, K, P, seed, p_done=0.3):
    """A random trajectory of pitch P, with step counts that reach the time
    limit inside it for some envs."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    B, n_o, n_u = env.num_envs, env.n_o, env.n_u

    def r(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    traj = {"obs": r(K, P, n_o)[:, :B], "term_obs": r(K, P, n_o)[:, :B], "u": r(K, P, n_u)[:, :B],
            "reward": r(K, P)[:, :B],
            "done": (torch.rand(K, P, device="cuda", generator=g) < p_done).to(torch.uint8)[:, :B]}
    obs0 = r(B, n_o)
    lim = env.max_episode_steps
    step0 = torch.randint(lim - K - 1, lim, (B,), device="cuda", generator=g, dtype=torch.int32)
    return traj, obs0, step0


def _assemble(env, traj, obs0, step0, K, auto_reset=True):
    """The K B records' fields, step-major, by the rules of rcbf_hip.h."""
    B = env.num_envs
    obs, u, rew = traj["obs"][:K], traj["u"][:K], traj["reward"][:K]
    done = traj["done"][:K] != 0
    term = traj.get("term_obs")
    prev = torch.cat([obs0[None], obs[:-1]], 0)
    nxt = obs.clone()
    if term is not None and auto_reset:
        nxt[done] = term[:K][done]
    c = step0.to(torch.int64).clone()
    mask, t, nt = [], [], []
    for j in range(K):
        e = c + 1
        mask.append(torch.where(e == env.max_episode_steps, torch.ones_like(e, dtype=torch.float64),
                                1.0 - done[j].to(torch.float64)))
        t.append(e.to(torch.float64) * env.dt)
        nt.append((e + 1).to(torch.float64) * env.dt)
        c = torch.where(done[j] & bool(auto_reset), torch.zeros_like(e), e)
    flat = lambda v, w=None: v.reshape(K * B, *(() if w is None else (w,)))  # noqa: E731
    return (flat(prev, env.n_o), flat(u, env.n_u), flat(rew), flat(nxt, env.n_o), flat(torch.stack(mask)),
            flat(torch.stack(t)), flat(torch.stack(nt)))


def _memories(env, capacity, position, size):
    """Two sentinel-filled rings at the same position."""
    from rcbf_amd.replay_memory import ReplayMemory
    out = []
    for _ in range(2):
        m = ReplayMemory(capacity, 3, device="cuda:0")
        m._dims = (env.n_o, env.n_u)
        m._ring = torch.full((capacity, m._width()), SENT, dtype=torch.float64, device="cuda")
        m.position, m._size = position, size
        out.append(m)
    return out


def _same(a, b):
    assert a.position == b.position and len(a) == len(b)
    ra, rb = a._ring.view(torch.int64), b._ring.view(torch.int64)
    if not torch.equal(ra, rb):
        bad = torch.nonzero(ra != rb)
        raise AssertionError(f"{bad.shape[0]} ring elements differ, first (slot, column) {bad[0].tolist()}")


def _case(mode, B, K, P, capacity, position, rows=None, term=True, auto_reset=True, seed=1):
    env = _Env(mode, B)
    alloc = K if rows is None else K + 2
    traj, obs0, step0 = _synthetic(env, alloc, P, seed)
    if not term:
        del traj["term_obs"]
    mem, twin = _memories(env, capacity, position, min(position, capacity))
    if term:
        mem.push_trajectory(env, traj, obs0, step0, rows=rows, auto_reset=auto_reset)
    else:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mem.push_trajectory(env, traj, obs0, step0, rows=rows, auto_reset=auto_reset)
    twin.batch_push(*_assemble(env, traj, obs0, step0, K, auto_reset))
    torch.cuda.synchronize()
    _same(mem, twin)
    return mem, twin


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
@pytest.mark.parametrize("B,P", [(1, 64), (63, 64), (65, 128), (130, 192)])
@pytest.mark.parametrize("K", [1, 5])
def test_ring_equals_batch_push(mode, B, P, K):
    """W = 25 and 19 (both odd): with an even and an odd position both
    alignments of a wave's first record occur; the ring is larger than the
    push, so the slots around it must keep the sentinel."""
    for position in (0, 7):
        _case(mode, B, K, P, K * B + 37, position, seed=B + K)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_wrap_inside_a_wave_and_next_to_a_record(mode):
    """B = 130, K = 5 (650 transitions): the ring's end falls inside a wave's 64
    records of some step, for every offset of the wrap within the wave's block
    that these positions reach -- its first record, its last, and between."""
    B, K, cap = 130, 5, 700
    for position in (cap - 1, cap - 64, cap - 65, cap - 130 - 33, cap - 2 * 130 - 64 - 1, cap - 649, cap - 650):
        _case(mode, B, K, 192, cap, position, seed=position)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
@pytest.mark.parametrize("capacity", [650, 649, 300, 64, 63, 10, 1])
def test_more_transitions_than_capacity(mode, capacity):
    """K B = 650 == capacity, and > capacity: the leading transitions are
    dropped, as sequential pushes leave the ring; down to a ring smaller than
    one wave's block."""
    for position in (0, capacity // 2, capacity - 1):
        _case(mode, 130, 5, 192, capacity, position, seed=capacity)


def test_rows_below_the_arrays_length_term_obs_none_and_auto_reset_false():
    _case("SimulatedCars", 65, 5, 128, 400, 3, rows=5)
    _case("Unicycle", 65, 3, 128, 400, 3, rows=3)
    _case("SimulatedCars", 65, 5, 128, 400, 3, term=False)
    _case("SimulatedCars", 65, 5, 128, 400, 3, auto_reset=False)
    _case("Unicycle", 65, 5, 128, 400, 3, term=False, auto_reset=False)


def test_a_warning_once_without_term_obs():
    env = _Env("SimulatedCars", 4)
    traj, obs0, step0 = _synthetic(env, 2, 64, 5)
    del traj["term_obs"]
    mem, _ = _memories(env, 50, 0, 0)
    with pytest.warns(UserWarning, match="term_obs"):
        mem.push_trajectory(env, traj, obs0, step0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mem.push_trajectory(env, traj, obs0, step0)  # once
        mem.push_trajectory(env, traj, obs0, step0, auto_reset=False)


def test_mask_at_the_time_limit_and_before_it():
    """Env 0 reaches step 300 with done set: mask 1 (main.py:105); env 1 is
    done at step 7: mask 0; env 2 is not done: mask 1."""
    env = _Env("SimulatedCars", 3)
    traj, obs0, step0 = _synthetic(env, 2, 64, 9)
    step0.copy_(torch.tensor([298, 5, 5], dtype=torch.int32))
    traj["done"].copy_(torch.tensor([[0, 0, 0], [1, 1, 0]], dtype=torch.uint8))
    mem, twin = _memories(env, 20, 0, 0)
    mem.push_trajectory(env, traj, obs0, step0)
    twin.batch_push(*_assemble(env, traj, obs0, step0, 2))
    _same(mem, twin)
    rec = mem._ring[3:6]
    assert rec[:, 22].tolist() == [1.0, 0.0, 1.0]
    assert rec[:, 23].tolist() == [300 * 0.02, 7 * 0.02, 7 * 0.02] and rec[0, 24].item() == 301 * 0.02
    want = torch.where(traj["done"][1].bool()[:, None], traj["term_obs"][1], traj["obs"][1]).double()
    assert torch.equal(rec[:, 12:22], want)


def test_ring_is_allocated_on_first_use_and_sampling_returns_pushed_rows():
    from rcbf_amd.replay_memory import ReplayMemory
    env = _Env("Unicycle", 65)
    traj, obs0, step0 = _synthetic(env, 4, 128, 21)
    mem = ReplayMemory(1000, 3, device="cuda:0")
    twin = ReplayMemory(1000, 3, device="cuda:0")
    mem.push_trajectory(env, traj, obs0, step0)
    twin.batch_push(*_assemble(env, traj, obs0, step0, 4))
    assert len(mem) == 260 == len(twin) and mem.position == 260 == twin.position
    assert torch.equal(mem._ring[:260].view(torch.int64), twin._ring[:260].view(torch.int64))
    got = torch.cat([v.reshape(64, -1) for v in mem.sample_tensors(64)], 1)
    rows = {tuple(r) for r in twin._ring[:260].cpu().numpy().view("int64").tolist()}
    assert all(tuple(r) in rows for r in got.cpu().numpy().view("int64").tolist())


def test_term_obs_plan_into_replay_end_to_end():
    """Cars, B = 65, K = 310: every env ends an episode inside the plan.  Every
    record with done set carries the terminal row as next_obs (not the reset
    row), and the same env's next record carries the reset row as obs_prev."""
    from rcbf_amd.aql import AqlQueue
    from rcbf_amd.replay_memory import ReplayMemory
    from test_gpu_aql_fused import _pool, _twins
    B, K = 65, 310
    (env, layer), = _twins("SimulatedCars", B, n=1)
    q = AqlQueue(torch.device("cuda", 0))
    try:
        traj = env.make_trajectory(K, ("obs", "u", "reward", "done", "term_obs"))
        traj["term_obs"]._base.fill_(SENT)
        obs0, step0 = env.obs.clone(), env.step_count.clone()
        plan = q.safe_step_plan(env, _pool(env, 7), layer, steps=K, trajectory=traj)
        plan.run()
        mem = ReplayMemory(K * B + 5, 0, device="cuda:0")
        mem.push_trajectory(env, traj, obs0, step0)
        twin = ReplayMemory(K * B + 5, 0, device="cuda:0")
        twin.batch_push(*_assemble(env, traj, obs0, step0, K))
        torch.cuda.synchronize()
        n = K * B
        assert len(mem) == n and mem.position == n
        assert torch.equal(mem._ring[:n].view(torch.int64), twin._ring[:n].view(torch.int64))
        rec = mem._ring[:n].view(K, B, 25)
        done = traj["done"].bool()
        assert int(done.sum()) >= B and bool(done.any(0).all())
        js, es = torch.nonzero(done[:K - 1], as_tuple=True)  # ... that have a next record in the plan
        assert js.numel() >= B
        assert torch.equal(rec[js, es, 12:22], traj["term_obs"][js, es].double())
        assert bool((rec[js, es, 12:22] != traj["obs"][js, es].double()).any(1).all())
        assert bool((traj["term_obs"][~done] == SENT).all()) and bool((traj["term_obs"][done] != SENT).all())
        assert torch.equal(rec[js + 1, es, 0:10], traj["obs"][js, es].double())
        assert bool((rec[js, es, 22] == 1.0).all()) and bool((rec[js, es, 23] == 300 * 0.02).all())
        assert bool((rec[js + 1, es, 23] == 1 * 0.02).all())
        plan.free()
    finally:
        q.close()


# Several steps per workgroup.  The shapes above give every workgroup ONE step (waves x K is far below 8 waves
# per CU), so the row and the count a lane carries from step to step, the barrier between two steps' records and
# a cut or a wrap at a step inside a chunk never run there.  B = 8 256 (129 waves) at pitch 8 320, K = 40: on a
# 256-CU device 14 chunks, 13 of 3 steps and the last of 1.  Every test asserts what it needs of the grid.
GRID_B, GRID_P, GRID_K = 8256, 8320, 40


def _grid_chunk():
    from _traj_grid import chunk
    c = chunk(GRID_B, GRID_K)
    assert 3 <= c < GRID_K and GRID_K % c == 1, c  # first, middle and last steps; the last chunk is one step
    return c


def _episode_steps(traj, step0, K, auto_reset=True):
    """e (K, B): the post-increment episode step of every transition, and done (K, B)."""
    done = traj["done"][:K] != 0
    c, e = step0.to(torch.int64).clone(), []
    for j in range(K):
        e.append(c + 1)
        c = torch.where(done[j] & bool(auto_reset), torch.zeros_like(c), e[-1])
    return torch.stack(e), done


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_several_steps_per_workgroup_equal_batch_push(mode):
    """Resets and the time limit land on first, middle and last steps of
    chunks: the row carried to the next step is the reset row (not the terminal
    row), the count carried is 0 after a reset."""
    B, P, K, seed = GRID_B, GRID_P, GRID_K, 61
    chunk = _grid_chunk()
    env = _Env(mode, B)
    traj, _, step0 = _synthetic(env, K, P, seed)  # what _case(seed=seed) packs
    e, done = _episode_steps(traj, step0, K)
    j = torch.arange(K, device="cuda")
    first, last = j % chunk == 0, (j % chunk == chunk - 1) | (j == K - 1)
    middle = ~first & ~last
    assert int(middle.sum()) >= K // chunk
    lim = e == env.max_episode_steps
    for where in (first, middle, last):  # (a middle step has a later step in its chunk)
        assert bool(done[where].any()) and bool(lim[where].any())
    # ... and an env is done on a middle step and again on a later step of the same chunk
    assert any(bool((done[m] & done[n]).any()) for m in torch.nonzero(middle)[:, 0].tolist()
               for n in range(m + 1, min((m // chunk + 1) * chunk, K)))
    for position in (0, 7):
        _case(mode, B, K, P, K * B + 37, position, seed=seed)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_several_steps_per_workgroup_without_term_obs(mode):
    """auto_reset=False: the count runs through done (every env reaches the
    time limit inside the plan); auto_reset=True without term_obs: next_obs is
    the reset row, the count restarts."""
    B, P, K, seed = GRID_B, GRID_P, GRID_K, 62
    chunk = _grid_chunk()
    env = _Env(mode, B)
    traj, _, step0 = _synthetic(env, K, P, seed)
    e, done = _episode_steps(traj, step0, K, auto_reset=False)
    at = torch.nonzero(e == env.max_episode_steps)[:, 0]  # the steps at which an env reaches the limit
    assert at.numel() >= B - B // 8 and {int(v) for v in (at % chunk).unique()} == set(range(chunk))
    assert bool(done[:-1].any())
    _case(mode, B, K, P, K * B + 37, 7, term=False, auto_reset=False, seed=seed)
    _case(mode, B, K, P, K * B + 37, 7, term=False, auto_reset=True, seed=seed)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_wrap_inside_a_chunk_of_several_steps(mode):
    """The ring's end falls inside the 64 records of wave w at step j, `head`
    of them before it: on the first, the middle and the last step of a chunk,
    after a wave's first record (head = 1) and before its last (head = 63)."""
    B, P, K = GRID_B, GRID_P, GRID_K
    chunk = _grid_chunk()
    cap, j0 = K * B + 37, 5 * chunk
    cuts = [(j0, 77, 33), (j0 + chunk // 2, 77, 33), (j0 + chunk - 1, 77, 33), (j0 + chunk // 2, 3, 1),
            (j0 + chunk // 2, 128, 63)]
    for j, w, head in cuts:
        position = cap - (j * B + 64 * w + head)
        assert 0 < position < cap and 0 < head < 64 and 64 * w + 64 <= B
        _case(mode, B, K, P, cap, position, seed=j + w)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_more_transitions_than_capacity_cuts_inside_a_chunk(mode):
    """capacity = K B - skip, the first kept transition inside a step in the
    middle of a chunk, on a chunk's first and last step, on a step's first row,
    on the last row before the one-step last chunk and inside it, and a
    one-slot ring; the ring starts empty and one slot before its end."""
    B, P, K = GRID_B, GRID_P, GRID_K
    chunk = _grid_chunk()
    mid, last = chunk + chunk // 2, K - 1
    assert 0 < mid % chunk < chunk - 1 and last % chunk == 0
    skips = [mid * B + 100, mid * B, chunk * B + 64 + 7, (2 * chunk - 1) * B + 4000, last * B + 5, last * B - 1,
             K * B - 1]
    for skip in skips:
        capacity = K * B - skip
        assert 0 < capacity < K * B
        for position in sorted({0, capacity - 1}):
            _case(mode, B, K, P, capacity, position, seed=skip % 1000)


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_a_last_wave_of_32_envs_with_several_steps_per_workgroup(mode):
    """8 256 and 65 600 are multiples of 64.  B = 8 224 at the same pitch and K
    (129 waves, the same chunks): the last wave holds 32 envs, its block of a
    step is 32 records; the ring wraps inside it on a chunk's middle step, and
    a cut falls inside it."""
    from _traj_grid import chunk as grid_chunk
    B, P, K = GRID_B - 32, GRID_P, GRID_K
    chunk = grid_chunk(B, K)
    assert chunk == _grid_chunk() and B % 64 == 32
    j, w = 4 * chunk + chunk // 2, B // 64
    cap = K * B + 37
    _case(mode, B, K, P, cap, cap - (j * B + 64 * w + 9), seed=71)
    skip = j * B + 64 * w + 9
    _case(mode, B, K, P, K * B - skip, 0, seed=72)


def test_the_flagship_grid_ten_steps_per_workgroup_cars():
    """B = 65 600 (1 025 waves) at pitch 65 664, K = 19: the grid training
    runs, two chunks of 10 and 9 steps on a 256-CU device; the ring wraps
    inside the last wave's records of step 4."""
    from _traj_grid import chunk
    B, P, K = 65600, 65664, 19
    assert 8 < chunk(B, K) < K
    cap = K * B + 37
    position = cap - (4 * B + 64 * 1024 + 9)
    assert 0 < position < cap and B == 64 * 1025
    mem, twin = _case("SimulatedCars", B, K, P, cap, position, seed=63)
    assert len(mem) == cap and mem.position == (position + K * B) % cap
    del mem._ring, twin._ring, mem, twin  # 250 MB each
    torch.cuda.empty_cache()
