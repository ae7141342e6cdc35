"""The SAC target on the device: DevicePolicy.sample (rcbf_policy_sample),
DeviceCritic.q / .td_target (rcbf_critic_q / rcbf_critic_td_target) and
sac_cbf.td_target, the block of rcbf_sac/sac_cbf.py:130-136.

Parity is against the fp64 port (tests/_critic_port.py).  No tolerance is fixed
in advance: each check computes e_ref, the max abs error of the reference
arithmetic (torch CPU fp32, as the reference writes it) against the port on the
same weights and inputs, and allows the kernel 8 e_ref + 1e-7 max|value|
(tests/test_gpu_policy.py says why x8).  log_pi is checked per row set, each
under its own allowance (_critic_port.row_sets): the rows whose pre-tanh values
stay below 4, those of them whose log_std is not near its lower clamp, and all
rows.  Where the tanh saturates, 1 - y^2 is rounding noise against the 1e-6
epsilon, and where std is tiny the reference's x_t - mean cancels, in the
reference as well: neither may dilute the tight check, and both are checked.
Every check prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import _critic_port as CP
import _policy_port as PP
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPES = {"cars": (10, 1), "unicycle": (7, 2), "wide": (16, 2)}  # wide: the 18-input critic, synthetic
CASES = [("cars", 32), ("cars", 64), ("cars", 256), ("unicycle", 32), ("unicycle", 64), ("unicycle", 256), ("wide", 32)]
MODES = {"cars": "SimulatedCars", "unicycle": "Unicycle"}
ROWS = (0, 63, 64, 129)


class Args:
    cuda = True


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def td_golden(golden, env):
    g = golden("td_target")
    psd = {k[len(env) + 5:]: v for k, v in g.items() if k.startswith(env + "_psd_")}
    csd = {k[len(env) + 5:]: v for k, v in g.items() if k.startswith(env + "_csd_")}
    d = {k[len(env) + 1:]: v for k, v in g.items() if k.startswith(env + "_")}
    return psd, csd, d, g


_CASES = {}


def case(golden, env, H):
    """Weights, 130 rows of inputs, the device objects and the port's and the torch restatement's outputs, built
    once per (env, H) and left unchanged."""
    if (env, H) in _CASES:
        return _CASES[env, H]
    from rcbf_amd.critic import DeviceCritic
    from rcbf_amd.policy import DevicePolicy
    n_o, n_u = SHAPES[env]
    rng = np.random.default_rng(1000 + H + n_o)
    if env != "wide" and H == 64:
        psd, csd, d, _ = td_golden(golden, env)
        scale, bias, obs = d["action_scale"], d["action_bias"], d["obs"]
    else:
        psd, csd = PP.seeded_weights(n_o, n_u, H, 100 + H), CP.seeded_critic(n_o + n_u, H, 200 + H)
        psd["log_std_linear.weight"] = psd["log_std_linear.weight"] * np.float32(4.0)
        scale, bias = np.full(n_u, 2.0, np.float32), np.linspace(0.5, -0.25, n_u).astype(np.float32)
        if env == "wide":
            real = rng.normal(0, 1, (65, n_o)).astype(np.float32)
            obs = np.concatenate([real, real * np.where(np.arange(65) % 2, -20.0, 20.0).astype(np.float32)[:, None]])
        else:
            obs = td_golden(golden, env)[2]["obs"]
    c = types_ns(psd=psd, csd=csd, scale=scale, bias=bias, obs=obs, n_o=n_o, n_u=n_u,
                 z=rng.normal(0, 1, (130, n_u)).astype(np.float32),
                 act=(rng.uniform(-1, 1, (130, n_u)) * scale + bias).astype(np.float32),
                 reward=rng.normal(0, 1, (130, 1)).astype(np.float32),
                 mask=rng.integers(0, 2, (130, 1)).astype(np.float32),
                 log_pi=rng.normal(-1, 2, (130, 1)).astype(np.float32), alpha=0.2, gamma=0.99)
    c.pol = DevicePolicy(PP.torch_module(psd, scale, bias), device="cuda")
    c.crit = DeviceCritic(CP.torch_critic(csd), device="cuda")
    c.want_sample = CP.sample(psd, scale, bias, obs, c.z)  # action, log_pi, mean, pre_tanh
    c.ref_sample = CP.torch_sample(psd, scale, bias, obs, c.z)
    c.ls = PP.forward(psd, obs)[1]
    c.want_q = CP.q_forward(csd, obs, c.act)
    c.ref_q = CP.torch_q(csd, obs, c.act)
    c.want_y = CP.target(c.reward, c.mask, c.gamma, *c.want_q, c.alpha, c.log_pi)
    c.ref_y = CP.torch_target(csd, obs, c.act, c.reward, c.mask, c.gamma, c.alpha, c.log_pi)
    _CASES[env, H] = c
    return c


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def run_sample(c, idx=slice(None), **kw):
    a, lp, m = c.pol.sample(dev(c.obs[idx]), z=dev(c.z[idx]), **kw)
    return host(a), host(lp), host(m)


def run_q(c, idx=slice(None)):
    q1, q2 = c.crit.q(dev(c.obs[idx]), dev(c.act[idx]))
    return host(q1), host(q2)


def run_td(c, idx=slice(None), alpha=None, **kw):
    return host(c.crit.td_target(dev(c.obs[idx]), dev(c.act[idx]), dev(c.reward[idx]), dev(c.mask[idx]),
                                 dev(c.log_pi[idx]), c.alpha if alpha is None else alpha, c.gamma, **kw))


@pytest.mark.parametrize("env,H", CASES)
def test_parity_with_the_port(golden, env, H):
    c = case(golden, env, H)
    tag = f"{env} H={H}"
    a, lp, m = run_sample(c)
    assert a.shape == (130, c.n_u) == m.shape and lp.shape == (130, 1)
    CP.check(tag + " action", a, c.ref_sample[0], c.want_sample[0])
    CP.check(tag + " mean action", m, c.ref_sample[2], c.want_sample[2])
    CP.check_log_pi(tag, lp[:, 0], c.ref_sample[1], c.want_sample[1], c.want_sample[3], c.ls)
    q1, q2 = run_q(c)
    assert q1.shape == (130, 1) == q2.shape
    CP.check(tag + " q1", q1[:, 0], c.ref_q[0], c.want_q[0])
    CP.check(tag + " q2", q2[:, 0], c.ref_q[1], c.want_q[1])
    y = run_td(c)
    assert y.shape == (130, 1)
    CP.check(tag + " y", y[:, 0], c.ref_y, c.want_y)


@pytest.mark.parametrize("env,H", [("cars", 64), ("unicycle", 256), ("unicycle", 32)])
def test_sample_is_bit_for_bit_the_existing_kernels(golden, env, H):
    c = case(golden, env, H)
    o, z = dev(c.obs), dev(c.z)
    a, lp, m = c.pol.sample(o, z=z)
    assert torch.equal(a.view(torch.int32), c.pol.act(o, evaluate=False, z=z).view(torch.int32))
    assert torch.equal(m.view(torch.int32), c.pol.act(o, evaluate=True).view(torch.int32))
    # the in-kernel draws, and the draw counter shared with act
    a2, lp2, _ = c.pol.sample(o, seed=77, counter=5)
    assert torch.equal(a2.view(torch.int32), c.pol.act(o, evaluate=False, seed=77, counter=5).view(torch.int32))
    assert torch.equal(c.pol.sample(o, seed=77, counter=5)[1].view(torch.int32), lp2.view(torch.int32))
    assert not torch.equal(c.pol.sample(o, seed=77, counter=6)[1], lp2)
    # ... whose log_pi is that of the oracle's draws (fp32 copies of the kernel's, an ulp apart at most: the port's
    # value for them, under the allowance of the port's check)
    zk = PP.draws(77, np.arange(130), 5, c.n_u)
    want = CP.sample(c.psd, c.scale, c.bias, c.obs, zk)
    CP.check_log_pi(f"{env} H={H} in-kernel draws", host(lp2)[:, 0], CP.torch_sample(c.psd, c.scale, c.bias, c.obs, zk)[1],
                    want[1], want[3], c.ls)
    c.pol._counter = 9
    a3 = c.pol.sample(o)[0]
    assert c.pol._counter == 10 and torch.equal(a3, c.pol.act(o, evaluate=False, counter=9))
    # into given tensors
    out = (torch.zeros(130, c.n_u, device="cuda"), torch.zeros(130, 1, device="cuda"), torch.zeros(130, c.n_u, device="cuda"))
    got = c.pol.sample(o, z=z, out=out)
    assert all(g is t for g, t in zip(got, out)) and torch.equal(out[1].view(torch.int32), lp.view(torch.int32))


@pytest.mark.parametrize("env,H", [("cars", 64), ("unicycle", 256), ("wide", 32)])
def test_a_row_does_not_depend_on_its_batch(golden, env, H):
    c = case(golden, env, H)
    _, lp, _ = run_sample(c)
    q1, q2 = run_q(c)
    y = run_td(c)
    assert np.array_equal(bits(y), bits(run_td(c)))  # two identical calls
    for i in ROWS:
        s = slice(i, i + 1)
        assert np.array_equal(bits(run_sample(c, s)[1]), bits(lp[s])), i
        one = run_q(c, s)
        assert np.array_equal(bits(one[0]), bits(q1[s])) and np.array_equal(bits(one[1]), bits(q2[s])), i
        assert np.array_equal(bits(run_td(c, s)), bits(y[s])), i
    perm = np.random.default_rng(5).permutation(130)[:65]
    assert np.array_equal(bits(run_sample(c, perm)[1]), bits(lp[perm]))
    assert np.array_equal(bits(run_td(c, perm)), bits(y[perm]))


@pytest.mark.parametrize("env,H", [("cars", 32), ("unicycle", 256), ("wide", 32)])
def test_the_64_row_tile_kernels(golden, env, H):
    """B just above 32 x CUs, where the launches switch to 64-row tiles (tests/test_gpu_policy.py): the rows are the
    130 repeated, so every row has a twin in the B = 130 call, which the 32-row kernels serve -- all outputs
    bit-equal to their twins, and the sentinel rows after row B intact."""
    c = case(golden, env, H)
    T = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    assert T % 64 == 0 and T >= 130
    a, lp, m = run_sample(c)
    q1, q2 = run_q(c)
    y = run_td(c)
    for B in (T + 1, T + 65):
        idx = np.arange(B) % 130
        nan = lambda w: torch.full((B + 64, w), float("nan"), device="cuda")  # noqa: E731
        ba, blp, bm, bq1, bq2, by, bq1t, bq2t = nan(c.n_u), nan(1), nan(c.n_u), nan(1), nan(1), nan(1), nan(1), nan(1)
        o, u = dev(c.obs[idx]), dev(c.act[idx])
        c.pol.sample(o, z=dev(c.z[idx]), out=(ba[:B], blp[:B], bm[:B]))
        c.crit.q(o, u, out=(bq1[:B], bq2[:B]))
        c.crit.td_target(o, u, dev(c.reward[idx]), dev(c.mask[idx]), dev(c.log_pi[idx]), c.alpha, c.gamma, out=by[:B],
                         q_out=(bq1t[:B], bq2t[:B]))
        for buf, small in ((ba, a), (blp, lp), (bm, m), (bq1, q1), (bq2, q2), (by, y), (bq1t, q1), (bq2t, q2)):
            h = host(buf)
            assert np.isnan(h[B:]).all() and np.array_equal(bits(h[B:]), bits(np.full_like(h[B:], np.nan))), B
            assert np.array_equal(bits(h[:B]), bits(small[idx])), B


@pytest.mark.parametrize("B", [1, 33, 130])
def test_rows_past_the_batch_are_untouched(golden, B):
    c = case(golden, "unicycle", 64)
    nan = lambda w: torch.full((B + 64, w), float("nan"), device="cuda")  # noqa: E731
    ba, blp, bm, bq1, bq2, by = nan(2), nan(1), nan(2), nan(1), nan(1), nan(1)
    s = slice(0, B)
    c.pol.sample(dev(c.obs[s]), z=dev(c.z[s]), out=(ba[:B], blp[:B], bm[:B]))
    c.crit.q(dev(c.obs[s]), dev(c.act[s]), out=(bq1[:B], bq2[:B]))
    c.crit.td_target(dev(c.obs[s]), dev(c.act[s]), dev(c.reward[s]), dev(c.mask[s]), dev(c.log_pi[s]), c.alpha, c.gamma,
                     out=by[:B])
    for buf in (ba, blp, bm, bq1, bq2, by):
        h = host(buf)
        assert np.all(np.isfinite(h[:B]))
        assert np.array_equal(bits(h[B:]), bits(np.full_like(h[B:], np.nan)))


def test_refresh_repacks_in_place_and_td_target_replays_under_a_graph(golden):
    from rcbf_amd.critic import DeviceCritic
    c = case(golden, "unicycle", 64)
    module = CP.torch_critic(c.csd).to("cuda")
    crit = DeviceCritic(module)
    assert crit.device.type == "cuda"
    o, u, r, k, lp = (dev(t) for t in (c.obs, c.act, c.reward, c.mask, c.log_pi))
    alpha = torch.tensor([c.alpha], device="cuda")
    before = crit.td_target(o, u, r, k, lp, alpha, c.gamma).clone()
    assert np.array_equal(bits(host(before)), bits(run_td(c)))
    ptr = crit.packed.data_ptr()
    with torch.no_grad():
        module.linear6.bias.add_(0.25)
        module.linear2.weight.mul_(0.5)
    assert torch.equal(crit.td_target(o, u, r, k, lp, alpha, c.gamma), before)  # packed: the module alone changes nothing
    # capture on the OLD weights, refresh, replay: one serial chain of one kernel, the packed buffer's address kept
    out = torch.zeros(130, 1, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        crit.td_target(o, u, r, k, lp, alpha, c.gamma, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crit.td_target(o, u, r, k, lp, alpha, c.gamma, out=out)
    crit.refresh()
    assert crit.packed.data_ptr() == ptr
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    after = crit.td_target(o, u, r, k, lp, alpha, c.gamma)
    assert torch.equal(out.view(torch.int32), after.view(torch.int32)) and not torch.equal(after, before)
    csd2 = {n: host(v.detach()) for n, v in module.state_dict().items()}
    want = CP.target(c.reward, c.mask, c.gamma, *CP.q_forward(csd2, c.obs, c.act), c.alpha, c.log_pi)
    ref = CP.torch_target(csd2, c.obs, c.act, c.reward, c.mask, c.gamma, c.alpha, c.log_pi)
    CP.check("refreshed y", host(after)[:, 0], ref, want)
    alpha.fill_(0.5)  # the device alpha is read when the graph runs
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), crit.td_target(o, u, r, k, lp, 0.5, c.gamma).view(torch.int32))


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_recorded_reference_outputs_stage_by_stage(golden, env):
    """Each stage on the stage's RECORDED inputs, so that its allowance is its own: the sample from the recorded
    eps; q1', q2' and y from the recorded safe action and log-probability."""
    c = case(golden, env, 64)
    psd, csd, d, g = td_golden(golden, env)
    alpha, gamma = float(g["alpha"]), float(g["gamma"])
    o = dev(d["obs"])
    a, lp, m = (host(t) for t in c.pol.sample(o, z=dev(d["eps"])))
    w_a, w_lp, w_m, pre = CP.sample(psd, d["action_scale"], d["action_bias"], d["obs"], d["eps"])
    for name, got, rec, want in (("action", a, d["action"], w_a), ("mean", m, d["mean"], w_m)):
        e_ref, allow = CP.bound(rec, want)
        err = float(np.max(np.abs(got - rec)))
        print(f"{env} {name} vs recorded: e_ref {e_ref:.3e} kernel-recorded {err:.3e} allowance {allow:.3e}")
        assert err <= allow, (name, err, allow)
    for what, rows in CP.row_sets(pre, c.ls):
        e_ref, allow = CP.bound(d["log_prob"][rows, 0], w_lp[rows])
        err = float(np.max(np.abs(lp[rows, 0] - d["log_prob"][rows, 0])))
        print(f"{env} log_pi vs recorded, {what}: e_ref {e_ref:.3e} kernel-recorded {err:.3e} allowance {allow:.3e}")
        assert rows.any() and err <= allow, (what, err, allow)
    safe = dev(d["safe"])
    assert (d["q1"] < d["q2"]).any() and (d["q2"] < d["q1"]).any()  # the min takes both sides
    q1, q2 = (host(t) for t in c.crit.q(o, safe))
    y = host(c.crit.td_target(o, safe, dev(d["reward"]), dev(d["mask"]), dev(d["log_prob"]), alpha, gamma))
    w_q1, w_q2 = CP.q_forward(csd, d["obs"], d["safe"])
    w_y = CP.target(d["reward"], d["mask"], gamma, w_q1, w_q2, alpha, d["log_prob"])
    for name, got, rec, want in (("q1", q1, d["q1"], w_q1), ("q2", q2, d["q2"], w_q2), ("next_q", y, d["next_q"], w_y)):
        e_ref, allow = CP.bound(rec[:, 0], want)
        err = float(np.max(np.abs(got[:, 0] - rec[:, 0])))
        print(f"{env} {name} vs recorded: e_ref {e_ref:.3e} kernel-recorded {err:.3e} allowance {allow:.3e}")
        assert err <= allow, (name, err, allow)


def _layer(env, g):
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv
    e = BatchedSimulatedCarsEnv(4) if env == "cars" else BatchedUnicycleEnv(4, hazards_locations=g["unicycle_hazards"])
    return CBFQPLayer(e, Args(), gamma_b=float(g["gamma_b"])), DynamicsModel(e, Args())


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_td_target_end_to_end(golden, env):
    """sac_cbf.td_target is the three public calls chained by hand, bit for bit, and lands within allowance of the
    reference's recorded next_q_value on every row: allowance 8 x |recorded - fp64 port chain| + 1e-6 max|y|.  Also
    the forms of alpha, diff_qp=False, and inputs as ReplayMemory.sample_tensors hands them out."""
    from rcbf_amd.sac_cbf import get_safe_action, td_target
    c = case(golden, env, 64)
    psd, csd, d, g = td_golden(golden, env)
    alpha, gamma = float(g["alpha"]), float(g["gamma"])
    layer, dyn = _layer(env, g)
    o, z, r, k = dev(d["obs"]), dev(d["eps"]), dev(d["reward"]), dev(d["mask"])
    y = td_target(c.pol, c.crit, layer, dyn, o, r, k, alpha, gamma, z=z)
    a, lp, _ = c.pol.sample(o, z=z)
    safe = get_safe_action(layer, o, a, dyn)
    by_hand = c.crit.td_target(o, safe, r, k, lp, alpha, gamma)
    assert y.shape == (130, 1) and torch.equal(y.view(torch.int32), by_hand.view(torch.int32))
    # the fp64 chain: port sample -> oracle safe action (on the fp32 action, as the layer takes it) -> port target
    w_a, w_lp, _, _ = CP.sample(psd, d["action_scale"], d["action_bias"], d["obs"], d["eps"])
    mode = MODES[env]
    mu, sg = O.predict_disturbance_prior(mode, 130)
    fin, aux = O.safe_action_diff(mode, O.get_state_f32(mode, d["obs"]), w_a.astype(np.float32), mu.astype(np.float32),
                                  sg.astype(np.float32), float(g["gamma_b"]),
                                  hazards=g["unicycle_hazards"] if env == "unicycle" else None)
    assert (aux["status"] == 0).all()
    w_y = CP.target(d["reward"], d["mask"], gamma, *CP.q_forward(csd, d["obs"], fin), alpha, w_lp)
    e_ref = float(np.max(np.abs(d["next_q"][:, 0] - w_y)))
    allow = 8.0 * e_ref + 1e-6 * float(np.max(np.abs(w_y)))
    err = float(np.max(np.abs(host(y)[:, 0] - d["next_q"][:, 0])))
    print(f"{env} end to end vs recorded next_q: e_ref {e_ref:.3e} kernel-recorded {err:.3e} allowance {allow:.3e}")
    assert err <= allow, (err, e_ref, allow)
    # alpha on the device; diff_qp=False skips the middle call
    y_dev = td_target(c.pol, c.crit, layer, dyn, o, r, k, torch.tensor(alpha, device="cuda"), gamma, z=z)
    assert torch.equal(y_dev.view(torch.int32), y.view(torch.int32))
    y_raw = td_target(c.pol, c.crit, layer, dyn, o, r, k, alpha, gamma, diff_qp=False, z=z)
    assert torch.equal(y_raw.view(torch.int32), c.crit.td_target(o, a, r, k, lp, alpha, gamma).view(torch.int32))
    if env == "cars":  # the filter moves some of the fixture's cars actions (none of the unicycle's), and the target with them
        assert not torch.equal(safe, a) and not torch.equal(y_raw, y)
    # strided fp64 views, (B,) reward and mask
    wide = torch.zeros(130, o.shape[1] + 3, dtype=torch.float64, device="cuda")
    wide[:, 1:1 + o.shape[1]] = o.double()
    y_view = td_target(c.pol, c.crit, layer, dyn, wide[:, 1:1 + o.shape[1]], r.double()[:, 0], k.double()[:, 0], alpha,
                       gamma, z=z)
    assert torch.equal(y_view.view(torch.int32), y.view(torch.int32))
    # in-kernel draws at a given counter
    y_c = td_target(c.pol, c.crit, layer, dyn, o, r, k, alpha, gamma, counter=3)
    a3, lp3, _ = c.pol.sample(o, counter=3)
    assert torch.equal(y_c, c.crit.td_target(o, get_safe_action(layer, o, a3, dyn), r, k, lp3, alpha, gamma))
