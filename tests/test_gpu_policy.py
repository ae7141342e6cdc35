"""The policy forward on the device (rcbf_policy_act through DevicePolicy) and
the closed-loop evaluation on top of it.

Parity is against the fp64 port (tests/_policy_port.py).  The tolerance is not
fixed in advance: each case computes e_ref, the max abs error of the reference
arithmetic (torch CPU fp32 F.linear / relu / tanh) against the port on the same
weights and inputs, and requires the kernel's max abs error <= 8 e_ref + 1e-7
scale.  The kernel sums each pre-activation as ONE chain of up to 256 terms,
whose worst-case bound is about K / block-length times that of torch's blocked
sums; x8 covers H = 256 against 8-16-wide partial sums, while a wrong column
or a dropped k-pair shows up at 1e-2.

Measured on an MI355X (max over B in {1, 33, 64, 65, 130}; e_ref / kernel error): see DESIGN 4.
"""
import numpy as np
import pytest
import torch

import _policy_port as PP
from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BATCHES = (1, 33, 64, 65, 130)  # one tile, a partial tile, an exact tile, tile + 1 row, two tiles + tail


class Args:
    cuda = True


def golden_case(golden, env):
    g = golden("policy")
    sd = {k[len(env) + 4:]: v for k, v in g.items() if k.startswith(env + "_sd_")}
    return sd, g[env + "_action_scale"], g[env + "_action_bias"], g


_CASES = {}


def case(golden, env, H):
    """(sd, scale, bias, obs (130, n_o), z (130, n_u), DevicePolicy), built once per (env, H)."""
    if (env, H) not in _CASES:
        from rcbf_amd.policy import DevicePolicy
        n_o, n_u = PP.ENV_SHAPES[env]
        gsd, gscale, gbias, g = golden_case(golden, env)
        if H == 64:
            sd, scale, bias = gsd, gscale, gbias
        else:  # generated in-test from a seed; a non-trivial affine map
            sd = PP.seeded_weights(n_o, n_u, H, 100 + H)
            scale, bias = np.full(n_u, 2.0, np.float32), np.linspace(0.5, -0.25, n_u).astype(np.float32)
        z = np.random.default_rng(H).normal(0, 1, (130, n_u)).astype(np.float32)
        pol = DevicePolicy(PP.torch_module(sd, scale, bias), device="cuda")
        _CASES[env, H] = (sd, scale, bias, g[env + "_obs"], z, pol)
    return _CASES[env, H]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def run(pol, obs, z=None, **kw):
    return pol.act(dev(obs), evaluate=z is None and "seed" not in kw, z=None if z is None else dev(z),
                   **kw).cpu().numpy()


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("H", [32, 64, 256])
@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_parity_with_the_port(golden, env, H, mode):
    sd, scale, bias, obs, z, pol = case(golden, env, H)
    for B in BATCHES:
        zz = z[:B] if mode == "sample" else None
        got = run(pol, obs[:B], zz)
        e_ref, bound = PP.bound(sd, scale, bias, obs[:B], zz)
        err = float(np.max(np.abs(got - PP.act(sd, scale, bias, obs[:B], zz))))
        print(f"policy parity {env} H={H} {mode} B={B}: e_ref {e_ref:.3e} kernel {err:.3e} bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and got.shape == (B, PP.ENV_SHAPES[env][1])
        assert err <= bound, (B, err, e_ref, bound)


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_parity_with_the_reference_recorded_outputs(golden, env):
    """H = 64 from the fixture, against GaussianPolicy.sample()[2] as the reference computed it."""
    sd, scale, bias, obs, _, pol = case(golden, env, 64)
    g = golden("policy")
    for B in BATCHES:
        got = run(pol, obs[:B])
        e_ref, bound = PP.bound(sd, scale, bias, obs[:B])
        err = float(np.max(np.abs(got.astype(np.float64) - g[env + "_action_mean"][:B])))
        print(f"policy vs recorded {env} B={B}: e_ref {e_ref:.3e} kernel {err:.3e} bound {bound:.3e}")
        assert err <= bound, (B, err, bound)


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("env,H", [("cars", 256), ("unicycle", 256), ("cars", 64), ("unicycle", 32)])
def test_a_row_does_not_depend_on_its_batch(golden, env, H, mode):
    sd, scale, bias, obs, z, pol = case(golden, env, H)
    zz = z if mode == "sample" else None
    whole = run(pol, obs, zz)
    assert np.array_equal(whole.view(np.uint32), run(pol, obs, zz).view(np.uint32))  # two identical calls
    for i in (0, 63, 64, 129):
        one = run(pol, obs[i:i + 1], None if zz is None else zz[i:i + 1])
        assert np.array_equal(one.view(np.uint32), whole[i:i + 1].view(np.uint32)), i
    # the same rows at other indices of a B = 65 batch
    perm = np.random.default_rng(5).permutation(130)[:65]
    moved = run(pol, obs[perm], None if zz is None else zz[perm])
    assert np.array_equal(moved.view(np.uint32), whole[perm].view(np.uint32))


def _tile_threshold():
    """The largest B that rcbf_policy_act still runs in 32-row tiles: 32 per CU of the device (8 192 on an
    MI355X); above it the 64-row kernels run."""
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("mode", ["mean", "sample"])
@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_the_64_row_tile_kernels(golden, env, H, mode):
    """B just above the threshold, where the launch switches to 64-row tiles: a last tile of 1 row, an exact
    tile, tile + 1 row, two tiles + 2 rows.  The rows are the fixture's 130 repeated, so every row has a twin
    in the B = 130 call, which the 32-row kernel serves: all rows bit-equal to their twins (the two kernels
    pinned to each other, every tile and row block of the large launch), parity with the port under the same
    bound, and the NaN guard rows after row B intact."""
    sd, scale, bias, obs, z, pol = case(golden, env, H)
    n_u = PP.ENV_SHAPES[env][1]
    T = _tile_threshold()
    assert T % 64 == 0 and T >= 130
    zz = z if mode == "sample" else None
    small = run(pol, obs, zz)  # B = 130: 32-row tiles
    want = PP.act(sd, scale, bias, obs, zz)
    e_ref, bound = PP.bound(sd, scale, bias, obs, zz)
    for B in (T + 1, T + 64, T + 65, T + 130):
        idx = np.arange(B) % 130
        buf = torch.full((B + 64, n_u), float("nan"), device="cuda")
        pol.act(dev(obs[idx]), evaluate=zz is None, z=None if zz is None else dev(zz[idx]), out=buf[:B])
        host = buf.cpu().numpy()
        got = host[:B]
        assert np.array_equal(host[B:].view(np.uint32), np.full((64, n_u), np.nan, np.float32).view(np.uint32)), B
        err = float(np.max(np.abs(got - want[idx])))
        print(f"policy parity, 64-row tiles {env} H={H} {mode} B={B}: e_ref {e_ref:.3e} kernel {err:.3e} "
              f"bound {bound:.3e}")
        assert np.all(np.isfinite(got)) and err <= bound, (B, err, bound)
        assert np.array_equal(got.view(np.uint32), small[idx].view(np.uint32)), B
        # and against single-row calls, first and last row of the batch
        for i in (0, B - 1):
            one = run(pol, obs[idx[i]:idx[i] + 1], None if zz is None else zz[idx[i]:idx[i] + 1])
            assert np.array_equal(one.view(np.uint32), got[i:i + 1].view(np.uint32)), (B, i)


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_in_kernel_draws_in_64_row_tiles(golden, env):
    """z == NULL above the threshold: the draws are the oracle's, and the last 65 rows equal the shard
    [T, T + 65) computed by the 32-row kernel with env_offset = T."""
    from rcbf_amd.policy import DevicePolicy
    sd, scale, bias, real, pol = _sampling_case(golden, env)
    n_u = PP.ENV_SHAPES[env][1]
    T = _tile_threshold()
    B, seed, counter = T + 65, 1234, 5
    obs = real[np.arange(B) % 65]
    got = run(pol, obs, seed=seed, counter=counter)
    want = run(pol, obs, PP.draws(seed, np.arange(B), counter, n_u))
    assert np.max(np.abs(got - want)) <= 4e-6 * scale.max()
    shard = DevicePolicy(pol.module, device="cuda", seed=seed, env_offset=T)
    part = run(shard, obs[T:], seed=seed, counter=counter)
    assert np.array_equal(part.view(np.uint32), got[T:].view(np.uint32))


def _sampling_case(golden, env):
    """Unsaturated inputs: the fixture's 65 real observations, tiled; small seeded weights (|mean| < 1, std ~ 1)."""
    from rcbf_amd.policy import DevicePolicy
    key = ("sampling", env)
    if key not in _CASES:
        n_o, n_u = PP.ENV_SHAPES[env]
        sd = PP.seeded_weights(n_o, n_u, 64, 7, gain=0.5)
        scale, bias = np.full(n_u, 2.0, np.float32), np.full(n_u, 0.5, np.float32)
        real = golden("policy")[env + "_obs"][:65]
        _CASES[key] = (sd, scale, bias, real, DevicePolicy(PP.torch_module(sd, scale, bias), device="cuda", seed=1234))
    return _CASES[key]


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_in_kernel_draws_are_the_model_steps(golden, env):
    sd, scale, bias, real, pol = _sampling_case(golden, env)
    n_u = PP.ENV_SHAPES[env][1]
    obs = np.tile(real, (2, 1))
    B, seed, counter = 130, 1234, 9
    got = run(pol, obs, seed=seed, counter=counter)
    z = PP.draws(seed, np.arange(B), counter, n_u)
    want = run(pol, obs, z)
    # |d tanh| <= 1: the bound on the pre-tanh scale bounds the action's at scale x
    assert np.max(np.abs(got - want)) <= 4e-6 * scale.max()
    y_got, y_want = (got - bias) / scale, (want - bias) / scale
    open_ = np.abs(y_want) < 0.9  # atanh amplifies the action's own fp32 rounding by 1 / (1 - y^2) beyond
    assert open_.mean() > 0.5
    assert np.max(np.abs(np.arctanh(y_got[open_].astype(np.float64)) - np.arctanh(y_want[open_].astype(np.float64)))) <= 4e-6
    # keyed by the counter and the seed; the default counter advances per call
    other = run(pol, obs, seed=seed, counter=counter + 1)
    assert not np.any(other == got)
    assert not np.any(run(pol, obs, seed=seed + 1, counter=counter) == got)
    pol._counter = counter
    assert np.array_equal(pol.act(dev(obs)).cpu().numpy(), got) and pol._counter == counter + 1
    assert np.array_equal(pol.act(dev(obs)).cpu().numpy(), other)
    # a shard draws what the whole batch would
    from rcbf_amd.policy import DevicePolicy
    shard = DevicePolicy(pol.module, device="cuda", seed=seed, env_offset=65)
    part = run(shard, obs[65:], seed=seed, counter=counter)
    assert np.array_equal(part.view(np.uint32), got[65:].view(np.uint32))


def test_in_kernel_draws_are_standard_normal(golden):
    sd, scale, bias, real, pol = _sampling_case(golden, "unicycle")
    B = 4096
    obs = np.tile(real, (B // 65 + 1, 1))[:B]
    u = run(pol, obs, seed=77, counter=3)
    z = PP.implied_z(sd, scale, bias, obs, u)
    assert np.all(np.isfinite(z))
    n = z.size
    st = O.normal_moments(z)
    se = 1.0 / np.sqrt(n)
    assert abs(st["mean"]) < 6 * se and abs(st["var"] - 1.0) < 6 * np.sqrt(2) * se, st
    assert abs(st["skew"]) < 6 * np.sqrt(6) * se and abs(st["exkurt"]) < 6 * np.sqrt(24) * se, st
    p3, p4 = 2.699796e-3, 6.334248e-5
    assert abs(st["p3"] - p3) < 6 * np.sqrt(p3 / n) and abs(st["p4"] - p4) < 6 * np.sqrt(p4 / n), st
    assert st["max"] <= np.sqrt(48 * np.log(2)) + 1e-2  # recovered through atanh of an fp32 action
    # and they are the oracle's draws, not merely normal
    assert np.max(np.abs(z - PP.draws(77, np.arange(B), 3, 2))) < 1e-2


@pytest.mark.parametrize("B", [1, 33, 130])
def test_rows_past_the_batch_are_untouched(golden, B):
    sd, scale, bias, obs, z, pol = case(golden, "unicycle", 64)
    for zz in (None, z[:B]):
        buf = torch.full((B + 64, 2), float("nan"), device="cuda")
        pol.act(dev(obs[:B]), evaluate=zz is None, z=None if zz is None else dev(zz), out=buf[:B])
        host = buf.cpu().numpy()
        assert np.all(np.isfinite(host[:B]))
        assert np.array_equal(host[B:].view(np.uint32), np.full((64, 2), np.nan, np.float32).view(np.uint32))


def test_refresh_repacks_in_place(golden):
    from rcbf_amd.policy import DevicePolicy
    sd, scale, bias, obs, _, _ = case(golden, "cars", 64)
    module = PP.torch_module(sd, scale, bias).to("cuda")
    pol = DevicePolicy(module)
    assert pol.device.type == "cuda"
    before = run(pol, obs)
    ptr = pol.packed.data_ptr()
    with torch.no_grad():
        module.mean_linear.bias.add_(0.25)
        module.linear2.weight.mul_(0.5)
    assert np.array_equal(run(pol, obs), before)  # packed weights: the module alone changes nothing
    pol.refresh()
    after = run(pol, obs)
    assert pol.packed.data_ptr() == ptr and not np.array_equal(after, before)
    sd2 = {k: v.detach().cpu().numpy() for k, v in module.state_dict().items()}
    e_ref, bound = PP.bound(sd2, scale, bias, obs)
    assert np.max(np.abs(after - PP.act(sd2, scale, bias, obs))) <= bound


@pytest.mark.parametrize("mode", ["mean", "sample"])
def test_act_replays_under_a_captured_graph(golden, mode):
    sd, scale, bias, obs, z, pol = case(golden, "unicycle", 256)
    o, out = dev(obs), torch.zeros(130, 2, device="cuda")
    zz = dev(z) if mode == "sample" else None
    eager = pol.act(o, evaluate=zz is None, z=zz).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pol.act(o, evaluate=zz is None, z=zz, out=out)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        pol.act(o, evaluate=zz is None, z=zz, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
    o.copy_(dev(obs[::-1].copy()))  # new inputs in the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), pol.act(o, evaluate=zz is None, z=zz).view(torch.int32))


def _make_env(env, B, seed):
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv
    if env == "cars":
        e = BatchedSimulatedCarsEnv(B, seed=seed)
    else:
        e = BatchedUnicycleEnv(B, seed=seed, hazards_locations=np.array([[0., 0.], [-1., 1.], [-1., -1.]]) * 1.5)
    return e, CBFQPLayer(e, Args(), gamma_b=20.0)


def _host_loop(env, pol, layer, steps):
    """policy.act + env.safe_step with the outputs copied out each step, the sums made in numpy fp64."""
    B = env.num_envs
    o = env.make_outputs()
    R, C, L = np.zeros(B), np.zeros(B), env.step_count.cpu().numpy().astype(np.int64)
    first = {"reward": np.full(B, np.nan), "cost": np.full(B, np.nan), "length": np.zeros(B, np.int32)}
    have = np.zeros(B, bool)
    for _ in range(steps):
        u = pol.act(env.obs, evaluate=True)
        env.safe_step(u, layer, outputs=o)
        R += o["reward"].cpu().numpy().astype(np.float64)
        C += o["cost"].cpu().numpy().astype(np.float64)
        L += 1
        done = o["done"].cpu().numpy().astype(bool)
        new = done & ~have
        first["reward"][new], first["cost"][new], first["length"][new] = R[new], C[new], L[new]
        have |= done
        R[done], C[done], L[done] = 0.0, 0.0, 0
    return first, have


@pytest.mark.parametrize("env,steps,reset", [("cars", 60, False), ("unicycle", 60, False), ("cars", 300, True)])
def test_evaluate_policy_is_the_host_loop(golden, env, steps, reset):
    """B = 65, H = 64.  steps = min(episode limit, 60) from step counts preloaded so that every env's
    episode ends inside the run, at a different step per env; and one whole cars episode from a reset."""
    from rcbf_amd.evaluator import _evaluate_from, evaluate_policy
    B = 65
    sd, scale, bias, _, _, pol = case(golden, env, 64)
    results = []
    for which in ("device", "host"):
        e, layer = _make_env(env, B, seed=21)
        if reset:
            if which == "host":
                e.reset()
        else:
            e.load_state(step=e.max_episode_steps - 2 - (np.arange(B) * 7) % 55)
        if which == "device":  # the public call resets; the preloaded cases enter its loop below the reset
            results.append(evaluate_policy(e, pol, layer, steps=steps) if reset
                           else _evaluate_from(e, pol, layer, steps))
        else:
            first, have = _host_loop(e, pol, layer, steps)
            e.check_failures()
    got = results[0]
    assert got["episodes"] == int(have.sum()) == B
    for f in ("reward", "cost"):
        assert np.array_equal(got[f].view(np.uint64), first[f].view(np.uint64)), f
    assert np.array_equal(got["length"], first["length"]) and got["length"].dtype == np.int32
    assert got["avg_reward"] == float(first["reward"].mean()) and got["avg_cost"] == float(first["cost"].mean())


def test_closed_loop_follows_the_port_and_the_oracle(golden):
    """Cars from the golden closed-loop start (env 32; the others +- 0.02 m/s apart): the device loop's
    policy action against the fp64 port stepping the C oracle, 20 steps, every env within the parity bound."""
    B = 65
    sd, scale, bias, _, _, pol = case(golden, "cars", 64)
    noise = float(golden("closed_loop_cars")["noise"]) + 0.02 * (np.arange(B) - 32)
    e, layer = _make_env("cars", B, seed=3)
    e.reset(noise=noise)
    x, t, st = O.cars_reset(noise)
    x, t, st = np.ascontiguousarray(x), t.astype(np.float64), st.astype(np.int32)
    obs = O.cars_obs(x).astype(np.float32)
    o = e.make_outputs()
    for k in range(20):
        u_dev = pol.act(e.obs, evaluate=True)
        got = u_dev.cpu().numpy()
        e.safe_step(u_dev, layer, outputs=o)
        want = PP.act(sd, scale, bias, obs)
        e_ref, bound = PP.bound(sd, scale, bias, obs)
        err = np.abs(got - want).max(axis=1)
        print(f"closed loop step {k}: e_ref {e_ref:.3e} max err {err.max():.3e} bound {bound:.3e}")
        assert int((err <= bound).sum()) == B, (k, np.flatnonzero(err > bound), err.max(), bound)
        out = CO.safe_step_ex("SimulatedCars", x, t, st, want.astype(np.float32), 20.0)
        assert out["fails"] == 0
        obs = out["obs"]
    e.check_failures()
