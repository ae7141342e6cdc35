"""rcbf_traj_episode_stats_f64 (k_traj_ep_count, k_traj_gp_scan,
k_traj_ep_pack) and rcbf_amd.EpisodeStats: per-episode return, cost and length
from the (K, B) reward, cost and done arrays of a trajectory plan.

The oracle is tests/_episode_port.py: a literal per-env Python loop of
main.py:98-101,140-144 with np.float64 accumulators, its records sorted
step-major, env-minor.  EVERYTHING is compared with np.array_equal, doubles as
their int64 bit patterns: fp32 widens exactly and the additions are made in
step order on both sides, so there is no tolerance in this feature.

Inputs are synthetic (the kernels do not care where they come from): reward and
cost randn * exp(4 randn) in fp32, done with p = 0.3, random len_in and a random
full-mantissa carry_in, in arrays of pitch P whose columns past B hold NaN and
done = 1 (a kernel that read them would show it).  Record arrays and carries
are sentinel-filled beyond what must be written.  One test runs a real plan."""
import functools
import types

import numpy as np
import pytest
import torch

from _episode_port import FIELDS, bits, episode_loop, same_records, synthetic

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -4321.25, -77
GRID = [(B, P, K) for (B, P) in ((1, 64), (63, 64), (65, 128), (130, 192)) for K in (1, 5, 37)] + [(64, 64, 600)]
SOME = [(1, 64, 1), (65, 128, 37), (130, 192, 5)]


@functools.lru_cache(maxsize=None)
def _inputs(B, K):
    """The numpy inputs of a shape: env 0 ends an episode at step K // 2, and
    (for B > 1) env B // 2 ends none."""
    s = synthetic(K, B, seed=1000 * B + K)
    s["done"][K // 2, 0] = 1
    if B > 1:
        s["done"][:, B // 2] = 0
    for v in s.values():
        v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(B, K, cost=True, carry=True, auto_reset=True, done="random"):
    s = _inputs(B, K)
    d = {"random": s["done"], "zero": np.zeros_like(s["done"]), "one": np.ones_like(s["done"])}[done]
    return episode_loop(s["reward"], s["cost"] if cost else None, d, s["carry"] if carry else None,
                        s["len"] if carry else None, auto_reset)


def _padded(a, P, pad, dtype):
    t = torch.full((a.shape[0], P), pad, dtype=dtype, device="cuda")
    t[:, :a.shape[1]] = torch.tensor(a, device="cuda")
    return t


def _run(B, P, K, cost=True, carry=True, auto_reset=True, done="random", max_rows=None, records=True, outs=True,
         slack=3):
    """One library call on the shape's inputs; every output as numpy, the
    record arrays `slack` rows longer than max_rows and the carries `slack`
    envs longer than B (sentinel-filled)."""
    from rcbf_amd import _lib
    lib = _lib.load()
    s = _inputs(B, K)
    d = {"random": s["done"], "zero": np.zeros_like(s["done"]), "one": np.ones_like(s["done"])}[done]
    rw, cs = _padded(s["reward"], P, float("nan"), torch.float32), _padded(s["cost"], P, float("nan"), torch.float32)
    dn = _padded(d, P, 1, torch.uint8)
    cin, lin = torch.tensor(s["carry"], device="cuda"), torch.tensor(s["len"], device="cuda")
    n_max = K * B if max_rows is None else max_rows
    rec_i = torch.full((3, n_max + slack), SENT_I, dtype=torch.int32, device="cuda")
    rec_f = torch.full((2, n_max + slack), SENT_F, dtype=torch.float64, device="cuda")
    cout = torch.full((B + slack, 2), SENT_F, dtype=torch.float64, device="cuda")
    lout = torch.full((B + slack,), SENT_I, dtype=torch.int32, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(lib.rcbf_traj_episode_stats_scratch_bytes(B, K) // 8, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    rows = [rec_i[0], rec_i[1], rec_i[2], rec_f[0], rec_f[1]] if records else [None] * 5
    rc = lib.rcbf_traj_episode_stats_f64(
        *(p(t) for t in rows), p(count), p(scratch), B, K, P, p(rw), p(cs if cost else None), p(dn),
        p(cin if carry else None), p(lin if carry else None), p(cout if outs else None), p(lout if outs else None),
        int(auto_reset), n_max, _lib.stream_of(torch.device("cuda", 0)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(zip(FIELDS, (t.cpu().numpy() for t in (*rec_i, *rec_f))))
    return got, count.cpu().numpy(), cout.cpu().numpy(), lout.cpu().numpy()


def _check(got, count, cout, lout, want, carry, length, max_rows=None):
    """Records [0, rows) equal the oracle's first rows; the sentinel beyond."""
    n_ep = want["env"].size
    rows = n_ep if max_rows is None else min(n_ep, max_rows)
    assert count.tolist() == [n_ep, rows]
    for f in FIELDS:
        assert np.array_equal(bits(got[f][:rows]), bits(want[f][:rows])), f
        sent = SENT_F if got[f].dtype == np.float64 else SENT_I
        assert got[f].size > rows and np.all(got[f][rows:] == sent), f
    B = length.size
    assert np.array_equal(bits(cout[:B]), bits(carry)) and np.all(cout[B:] == SENT_F)
    assert np.array_equal(lout[:B], length) and np.all(lout[B:] == SENT_I)


@pytest.mark.parametrize("B,P,K", GRID)
def test_records_counts_and_carries_equal_the_loop(B, P, K):
    want, carry, length = _oracle(B, K)
    done = _inputs(B, K)["done"]
    assert want["env"].size == done.sum() >= 1  # an episode ends inside the run ...
    assert B == 1 or not done.any(0).all()      # ... and an env ends none: its sums only run into the carry
    open_before = want["length"] > want["step"]  # episodes that were open before the run, and ones begun inside it
    assert K < 37 or (open_before.any() and not open_before.all())
    _check(*_run(B, P, K), want, carry, length)


@pytest.mark.parametrize("B,P,K", SOME)
def test_no_done_byte_no_episode(B, P, K):
    s = _inputs(B, K)
    want, carry, length = _oracle(B, K, done="zero")
    assert want["env"].size == 0 and np.array_equal(length, s["len"] + K)
    run = np.cumsum(np.concatenate([s["carry"][None, :, 0], s["reward"].astype(np.float64)]), 0)[-1]
    assert np.array_equal(bits(carry[:, 0]), bits(run))  # the running sums
    _check(*_run(B, P, K, done="zero"), want, carry, length)


@pytest.mark.parametrize("B,P,K", SOME)
def test_every_step_ends_an_episode(B, P, K):
    s = _inputs(B, K)
    want, carry, length = _oracle(B, K, done="one")
    got, count, cout, lout = _run(B, P, K, done="one")
    assert count.tolist() == [K * B, K * B]
    assert np.array_equal(got["length"][:B], s["len"] + 1) and np.all(got["length"][B:K * B] == 1)
    assert not cout[:B].any() and not lout[:B].any()
    _check(got, count, cout, lout, want, carry, length)


@pytest.mark.parametrize("B,P,K", SOME)
def test_without_auto_reset_the_sums_run_through_done(B, P, K):
    s = _inputs(B, K)
    want, carry, length = _oracle(B, K, auto_reset=False)
    assert s["done"].any() and want["env"].size == 0 and np.array_equal(length, s["len"] + K)
    _check(*_run(B, P, K, auto_reset=False), want, carry, length)


@pytest.mark.parametrize("B,P,K", SOME)
def test_without_cost_the_cost_column_is_the_carry_then_zero(B, P, K):
    s = _inputs(B, K)
    want, carry, length = _oracle(B, K, cost=False)
    first = want["length"] > want["step"]  # the episode was open before the run
    assert first.any() and np.array_equal(bits(want["cost"][first]), bits(s["carry"][want["env"][first], 1]))
    assert not want["cost"][~first].any()
    _check(*_run(B, P, K, cost=False), want, carry, length)


@pytest.mark.parametrize("B,P,K", SOME)
def test_null_carry_and_lengths_are_zeros(B, P, K):
    want, carry, length = _oracle(B, K, carry=False)
    assert np.all(want["length"] <= want["step"] + 1)
    _check(*_run(B, P, K, carry=False), want, carry, length)


@pytest.mark.parametrize("B,P,K", [(65, 128, 37), (130, 192, 5)])
def test_max_rows_keeps_the_first_and_reports_the_total(B, P, K):
    want, carry, length = _oracle(B, K)
    n_ep = want["env"].size
    for max_rows in (1, n_ep // 2, n_ep - 1):
        assert 0 < max_rows < n_ep
        _check(*_run(B, P, K, max_rows=max_rows), want, carry, length, max_rows=max_rows)


@pytest.mark.parametrize("B,P,K", SOME)
def test_count_only_call_with_null_records_and_null_outs(B, P, K):
    want, carry, length = _oracle(B, K)
    got, count, cout, lout = _run(B, P, K, max_rows=0, records=False, outs=False)
    assert count.tolist() == [want["env"].size, 0]
    assert np.all(cout == SENT_F) and np.all(lout == SENT_I)  # nothing is advanced
    # ... and with the outs given, the carries advance though no record is kept
    _check(*_run(B, P, K, max_rows=0, records=False), want, carry, length, max_rows=0)


def test_the_same_call_twice_gives_the_same_bits():
    B, P, K = 130, 192, 37
    a, b = _run(B, P, K), _run(B, P, K)
    assert all(np.array_equal(bits(a[0][f]), bits(b[0][f])) for f in FIELDS)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))


def _stats(B, K, P=None):
    """An EpisodeStats on the shape's inputs (its carry set to theirs) and the
    trajectory as [:, :B] views of pitch P."""
    from rcbf_amd import EpisodeStats
    s = _inputs(B, K)
    env = types.SimpleNamespace(num_envs=B, step_count=torch.tensor(s["len"], device="cuda"))
    stats = EpisodeStats(env)
    stats.running()[0].copy_(torch.tensor(s["carry"], device="cuda"))
    P = P or B
    traj = {"reward": _padded(s["reward"], P, float("nan"), torch.float32)[:, :B],
            "cost": _padded(s["cost"], P, float("nan"), torch.float32)[:, :B],
            "done": _padded(s["done"], P, 1, torch.uint8)[:, :B]}
    return stats, traj


def _numpy(out):
    return {f: out[f].cpu().numpy() for f in FIELDS}


@pytest.mark.parametrize("B,P,K,K1", [(130, 192, 37, 20), (65, 128, 37, 1), (64, 64, 600, 333)])
def test_two_updates_over_the_halves_equal_one_over_the_whole(B, P, K, K1):
    want, carry, length = _oracle(B, K)
    stats, traj = _stats(B, K, P)
    whole = stats.update(traj)
    assert whole["n_episodes"] == want["env"].size == whole["env"].shape[0]
    assert same_records(_numpy(whole), want)
    assert np.array_equal(bits(stats.running()[0].cpu().numpy()), bits(carry))
    assert np.array_equal(stats.running()[1].cpu().numpy(), length)
    stats, traj = _stats(B, K, P)
    a = stats.update(traj, rows=K1)
    mid = stats.running()[0].cpu().numpy()
    b = stats.update({f: t[K1:] for f, t in traj.items()})
    assert a["n_episodes"] > 0 and b["n_episodes"] > 0 and mid.any()  # both halves end episodes; a carry crosses
    a, b = _numpy(a), _numpy(b)
    b["step"] = b["step"] + K1
    assert same_records({f: np.concatenate([a[f], b[f]]) for f in FIELDS}, want)
    assert np.array_equal(bits(stats.running()[0].cpu().numpy()), bits(carry))
    assert np.array_equal(stats.running()[1].cpu().numpy(), length)


def test_max_episodes_is_one_call_and_trims_when_looked_at():
    B, P, K = 130, 192, 5
    want, carry, length = _oracle(B, K)
    n_ep = want["env"].size
    for cap in (n_ep + 7, n_ep // 2):
        stats, traj = _stats(B, K, P)
        out = stats.update(traj, max_episodes=cap)
        assert out["env"].shape[0] == cap and "n_episodes" not in out
        assert out["n_episodes"] == n_ep and out["count"].tolist() == [n_ep, min(n_ep, cap)]
        got = _numpy(out)
        assert all(np.array_equal(bits(got[f]), bits(want[f][:cap])) for f in FIELDS)
        assert np.array_equal(bits(stats.running()[0].cpu().numpy()), bits(carry))  # truncation loses no sum


def test_one_step_output_buffers_are_a_one_row_trajectory():
    """K = 1, P = B: the policy-in-the-loop use, step by step, against the loop
    over the whole array."""
    B, K = 65, 5
    s = _inputs(B, K)
    want, carry, length = _oracle(B, K)
    stats, _ = _stats(B, K)
    got = {f: [] for f in FIELDS}
    for j in range(K):
        out = {"reward": torch.tensor(s["reward"][j], device="cuda"),
               "cost": torch.tensor(s["cost"][j], device="cuda"), "done": torch.tensor(s["done"][j], device="cuda")}
        rec = stats.update({f: t[None] for f, t in out.items()})
        assert not rec["step"].any()
        for f in FIELDS:
            got[f].append(rec[f].cpu().numpy() + (j if f == "step" else 0))
    assert same_records({f: np.concatenate(v) for f, v in got.items()}, want)
    assert np.array_equal(bits(stats.running()[0].cpu().numpy()), bits(carry))
    assert np.array_equal(stats.running()[1].cpu().numpy(), length)


def test_a_real_cars_plan_ends_one_episode_of_300_steps_per_env():
    from rcbf_amd import EpisodeStats
    from rcbf_amd.aql import AqlQueue
    from test_gpu_aql_fused import _pool
    from test_gpu_headline_parity import _make
    B, K = 130, 310
    env, layer = _make("SimulatedCars", B)
    assert not env.step_count.any()  # a fresh reset
    q = AqlQueue(torch.device("cuda", 0))
    try:
        traj = env.make_trajectory(K, ("reward", "cost", "done"))
        stats = EpisodeStats(env)
        plan = q.safe_step_plan(env, _pool(env, 7), layer, steps=K, trajectory=traj)
        plan.run()
        torch.cuda.synchronize()
        out = stats.update(traj)
        plan.free()
    finally:
        q.close()
    rw, cs, dn = (traj[f].cpu().numpy() for f in ("reward", "cost", "done"))
    want, carry, length = episode_loop(rw, cs, dn)
    assert out["n_episodes"] == B and np.array_equal(want["env"], np.arange(B))  # one episode per env ...
    assert np.all(want["length"] == 300) and np.all(want["step"] == 299)         # ... at the time limit
    assert same_records(_numpy(out), want)
    assert np.unique(want["reward"]).size > 1  # the envs' returns differ
    run, steps = stats.running()
    assert np.array_equal(bits(run.cpu().numpy()), bits(carry))
    assert torch.equal(steps, env.step_count) and np.all(length == K - 300)


@pytest.fixture
def _large_shapes_leave_the_caches():
    """The inputs and the oracle's records of a large shape are not kept for
    the rest of the session."""
    yield
    _inputs.cache_clear()
    _oracle.cache_clear()


@pytest.mark.parametrize("B,P,K", [(8256, 8320, 40), (8224, 8320, 40), (65600, 65664, 19)])
def test_several_steps_per_workgroup_equal_the_loop(B, P, K, _large_shapes_leave_the_caches):
    """GRID gives every workgroup of the count pass ONE step (waves x K is far
    below 8 waves per CU), so only lane 0 of its 8-step batch ever holds a live
    step.  (8 256, 40): chunks of 3 steps on a 256-CU device, the last of 1.
    (8 224, 40): the same grid with a last wave of 32 envs beside the NaN /
    done = 1 padding (8 256 and 65 600 are multiples of 64).  (65 600, 19), the
    grid training runs: chunks of 10 and 9 steps -- a full batch of 8 and a
    tail -- and 1 025 x 19 = 19 475 counts, two tiles of the scan.  The full
    call with carries in and out, and max_rows at half the episodes and inside
    the last wave's records of a step in the middle of a chunk."""
    from _traj_grid import chunk as grid_chunk
    chunk, waves = grid_chunk(B, K), (B + 63) // 64
    assert 1 < chunk < K
    if K == 40:
        assert chunk < 8 and K % chunk  # a partly filled batch; a shorter last chunk
        assert B % 64 == (32 if B == 8224 else 0)
    else:
        assert chunk > 8 and chunk % 8 and waves * K > 16384
    want, carry, length = _oracle(B, K)
    n_ep = want["env"].size
    assert n_ep == _inputs(B, K)["done"].sum() > K * B // 4
    _check(*_run(B, P, K), want, carry, length)
    j = chunk + chunk // 2  # a step that is neither its chunk's first nor its last
    assert 0 < j % chunk < chunk - 1 and j < K
    here = np.nonzero((want["step"] == j) & (want["env"] // 64 == waves - 1))[0]
    assert here.size >= 2 and np.array_equal(here, np.arange(here[0], here[0] + here.size))
    inside = int(here[0]) + here.size // 2
    assert here[0] < inside <= here[-1]
    for max_rows in (n_ep // 2, inside):
        _check(*_run(B, P, K, max_rows=max_rows), want, carry, length, max_rows=max_rows)
