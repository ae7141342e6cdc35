"""SURVEY 8f rows 3-4 on the GPU: the model-rollout step kernel against the
reference's own generate_model_rollouts outputs (tests/golden/model_rollouts.npz,
recorded N(0,1) draws replayed), and the device ReplayMemory against the
reference's list semantics."""
import types

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _env(mode):
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv
    return BatchedSimulatedCarsEnv(4) if mode == "SimulatedCars" else BatchedUnicycleEnv(4)


@pytest.mark.parametrize("nm,mode", [("cars", "SimulatedCars"), ("uni", "Unicycle")])
def test_model_step_vs_reference(golden, nm, mode):
    from rcbf_amd.generate_rollouts import model_step
    d = golden("model_rollouts")
    nobs, r, mask, nt = model_step(_env(mode), d[nm + "_obs"], d[nm + "_act"], d[nm + "_t"], z=d[nm + "_z"])
    assert np.max(np.abs(nobs.cpu().numpy() - d[nm + "_next_obs"])) <= 1e-12
    assert np.max(np.abs(r.cpu().numpy() - d[nm + "_reward"])) <= 1e-12
    assert np.array_equal(mask.cpu().numpy(), d[nm + "_mask"])
    assert np.array_equal(nt.cpu().numpy(), d[nm + "_next_t"])


def test_model_step_philox_noise_and_gp_mean():
    """In-kernel N(0,1) draws are standard normal and keyed by the counter;
    a GP mean/std enters as mu + dt mean, std dt std (oracle)."""
    from rcbf_amd.generate_rollouts import model_step
    rng = np.random.default_rng(4)
    B = 65536
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-np.pi, np.pi, B)], 1)
    obs = O.uni_obs(x)
    act = rng.uniform(-1, 1, (B, 2))
    env = _env("Unicycle")
    n1, *_ = model_step(env, obs, act, z=None, seed=5, counter=0)
    n2, *_ = model_step(env, obs, act, z=None, seed=5, counter=0)
    n3, *_ = model_step(env, obs, act, z=None, seed=5, counter=1)
    assert torch.equal(n1, n2) and not torch.equal(n1, n3)
    base, *_ = model_step(env, obs, act, z=np.zeros((B, 3)))
    zhat = ((n1 - base)[:, :2].cpu().numpy()) / (0.02 * 0.2)
    assert abs(zhat.mean()) < 0.02 and abs(zhat.std() - 1.0) < 0.02
    mean = rng.normal(0, 0.1, (B, 3)).astype(np.float32)
    std = rng.uniform(0.01, 0.3, (B, 3)).astype(np.float32)
    z = rng.normal(0, 1, (B, 3))
    nobs, r, mask, nt = model_step(env, obs, act, mean=mean, std=std, z=z)
    on, orr, om, ot = O.model_rollout_step("Unicycle", obs, act, None, z, mean=mean, std=std)
    assert np.max(np.abs(nobs.cpu().numpy() - on)) <= 1e-12 and np.max(np.abs(r.cpu().numpy() - orr)) <= 1e-12


def _assert_standard_normal(st, n):
    """Moment and tail bounds at about 6 standard errors for n samples."""
    se = 1.0 / np.sqrt(n)
    assert abs(st["mean"]) < 6 * se and abs(st["var"] - 1.0) < 6 * np.sqrt(2) * se, st
    assert abs(st["skew"]) < 6 * np.sqrt(6) * se and abs(st["exkurt"]) < 6 * np.sqrt(24) * se, st
    p3, p4 = 2.699796e-3, 6.334248e-5  # P(|z| > 3), P(|z| > 4) of N(0, 1)
    assert abs(st["p3"] - p3) < 6 * np.sqrt(p3 / n) and abs(st["p4"] - p4) < 6 * np.sqrt(p4 / n), st
    assert st["max"] <= np.sqrt(48 * np.log(2)) + 1e-6, st  # 24-bit uniforms: |z| <= 5.768


def test_model_step_draw_moments_tails_and_key():
    """The in-kernel N(0, 1) draws of rcbf_model_step (fp32 Box-Muller on
    24-bit Philox uniforms, hardware log2 / cos / sin) against the reference's
    np.random.normal (generate_rollouts.py:31; fp64, values unpinned): over
    2^20 rows x 4 counters x 2 recoverable components (8.4 M samples) the mean,
    variance, skewness, excess kurtosis and the P(|z| > 3), P(|z| > 4) tails
    sit within 6 standard errors of N(0, 1), and |z| never exceeds the
    truncation bound sqrt(48 ln 2) = 5.768.  The first 4096
    rows equal the oracle's restatement of the keyed draw
    (oracle.model_step_normal) to 2e-5."""
    from rcbf_amd.generate_rollouts import model_step
    rng = np.random.default_rng(6)
    B = 1 << 20
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-np.pi, np.pi, B)], 1)
    obs = O.uni_obs(x)
    act = rng.uniform(-1, 1, (B, 2))
    env = _env("Unicycle")
    base, *_ = model_step(env, obs, act, z=np.zeros((B, 3)))
    zs = []
    for counter in range(4):
        n1, *_ = model_step(env, obs, act, z=None, seed=11, counter=counter)
        z = ((n1 - base)[:, :2] / (0.02 * 0.2)).cpu().numpy()  # obs[:, :2] = next x, y = mu + dt sd z
        zs.append(z)
        if counter == 1:
            want = O.model_step_normal(11, np.arange(4096), counter, 3)[:, :2]
            assert np.max(np.abs(z[:4096] - want)) <= 2e-5
    zs = np.concatenate(zs)
    _assert_standard_normal(O.normal_moments(zs), zs.size)


def test_replay_memory_ring_and_sample():
    from rcbf_amd.replay_memory import ReplayMemory
    rng = np.random.default_rng(0)
    mem = ReplayMemory(100, seed=1)
    ref = []  # the reference's list semantics (replay_memory.py:12-21)
    pos = 0
    for n in (30, 50, 45, 7, 130):
        s = rng.normal(size=(n, 10)); a = rng.normal(size=(n, 1)); r = rng.normal(size=n)
        ns = rng.normal(size=(n, 10)); m = rng.integers(0, 2, n).astype(bool); t = rng.normal(size=n)
        mem.batch_push(s, a, r, ns, m, t, t + 0.02)
        for i in range(n):
            rec = np.concatenate([s[i], a[i], [r[i]], ns[i], [float(m[i])], [t[i]], [t[i] + 0.02]])
            if len(ref) < 100:
                ref.append(None)
            ref[pos] = rec
            pos = (pos + 1) % 100
        assert len(mem) == len(ref) and mem.position == pos
    ring = mem._ring.cpu().numpy()
    assert np.array_equal(ring, np.stack(ref))
    S, A, R, NS, M, T, NT = mem.sample(64)
    rows = np.hstack([S, A, R[:, None], NS, M[:, None], T[:, None], NT[:, None]])
    keys = {r.tobytes() for r in np.stack(ref)}
    assert all(r.tobytes() in keys for r in rows) and len({r.tobytes() for r in rows}) == 64  # no replacement
    with pytest.raises(ValueError):
        mem.sample(101)
    mem.push(s[0], a[0], r[0], ns[0], m[0])  # single push without t
    assert len(mem) == 100


def test_generate_model_rollouts_end_to_end():
    """generate_model_rollouts with device memories and a host policy:
    every pushed transition equals the oracle step on the sampled batch."""
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.generate_rollouts import generate_model_rollouts
    from rcbf_amd.replay_memory import ReplayMemory
    env = _env("SimulatedCars")
    rng = np.random.default_rng(2)
    mem = ReplayMemory(1000, seed=3)
    B = 500
    st = np.tile(np.array([34.0, 30.0, 28.0, 30.0, 22.0, 30.0, 16.0, 35.0, 10.0, 30.0]), (B, 1)) + rng.normal(0, 1, (B, 10))
    obs = st.copy(); obs[:, ::2] /= 100.0; obs[:, 1::2] /= 30.0
    t = np.round(rng.uniform(0, 6, B) / 0.02) * 0.02
    mem.batch_push(obs, rng.uniform(-1, 1, (B, 1)), np.zeros(B), obs, np.ones(B), t, t + 0.02)

    class Agent:
        def select_action(self, o, dm, warmup=False, evaluate=False):
            return np.clip(o[:, 7:8] * 2 - 2, -1, 1)

    mm = ReplayMemory(1000, seed=4)
    dm = DynamicsModel(env, types.SimpleNamespace(cuda=True, gp_model_size=100))
    generate_model_rollouts(env, mm, mem, Agent(), dm, k_horizon=1, batch_size=200)
    assert len(mm) == 200
    S, A, R, NS, M, T, NT = (v.cpu().numpy() for v in mm.sample_tensors(200))
    assert np.allclose(A, np.clip(S[:, 7:8] * 2 - 2, -1, 1))
    # replay each transition through the oracle with the kernel's own draws recovered from NS
    base, rb, mb, tb = O.model_rollout_step("SimulatedCars", S, A, T, np.zeros((200, 10)))
    assert np.max(np.abs(R - rb)) <= 1e-12 and np.array_equal(M, mb) and np.array_equal(NT, tb)
    zh = (NS - base)[:, 1::2] * 30.0 / (0.02 * 0.2)
    assert np.all(np.abs(zh) < 7) and np.array_equal(NS[:, ::2], base[:, ::2])


@pytest.mark.parametrize("nm,mode", [("cars", "SimulatedCars"), ("uni", "Unicycle")])
def test_predict_next_state_device_vs_reference(golden, nm, mode):
    """DynamicsModel.predict_next_state on device tensors (the
    rcbf_predict_next_state kernel) against the reference's own outputs
    (tests/golden/dynamics.npz, use_gps=False: bit-exact), the MAX_STD prior
    (use_gps=True before a fit: dt * MAX_STD, mean 0), a GP posterior's
    (mean, std) entering as next + dt * mean, dt * std, and the 1-D form."""
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import SimulatedCarsEnv, UnicycleEnv
    d = golden("dynamics")
    env = SimulatedCarsEnv() if mode == "SimulatedCars" else UnicycleEnv()
    dm = DynamicsModel(env, types.SimpleNamespace(cuda=True, gp_model_size=2000))
    dev = torch.device("cuda", 0)
    x = torch.as_tensor(d[nm + "_state_np"], device=dev)
    u = torch.as_tensor(d[nm + "_u"], device=dev)
    t = torch.as_tensor(d[nm + "_t"], device=dev) if nm + "_t" in d else None
    nx, sd, nt = dm.predict_next_state(x, u, t_batch=t, use_gps=False)
    assert nx.is_cuda and np.array_equal(nx.cpu().numpy(), d[nm + "_next"])
    assert not sd.cpu().numpy().any()
    if t is not None:
        assert np.array_equal(nt.cpu().numpy(), d[nm + "_t"] + 0.02)
    # the prior: mean 0, std dt * MAX_STD (the numpy path of the same class agrees)
    nx2, sd2, _ = dm.predict_next_state(x, u, t_batch=t, use_gps=True)
    ref_nx, ref_sd, _ = dm.predict_next_state(d[nm + "_state_np"], d[nm + "_u"],
                                              t_batch=d.get(nm + "_t"), use_gps=True)
    assert np.array_equal(nx2.cpu().numpy(), ref_nx) and np.array_equal(sd2.cpu().numpy(), ref_sd)
    _, s_prior = O.predict_disturbance_prior(mode, x.shape[0])
    assert np.array_equal(sd2.cpu().numpy(), 0.02 * s_prior)
    # a fitted GP's posterior (stand-in estimator returning fixed f32 mean / std)
    rng = np.random.default_rng(11)
    m32 = rng.normal(0, 0.05, x.shape).astype(np.float32)
    s32 = rng.uniform(0.01, 0.3, x.shape).astype(np.float32)

    class _GP:
        def predict(self, xq):
            return torch.as_tensor(m32, device=xq.device), torch.as_tensor(s32, device=xq.device)
    dm.disturb_estimators = _GP()
    nx3, sd3, _ = dm.predict_next_state(x, u, t_batch=t, use_gps=True)
    assert np.array_equal(nx3.cpu().numpy(), d[nm + "_next"] + 0.02 * m32.astype(np.float64))
    assert np.array_equal(sd3.cpu().numpy(), 0.02 * s32.astype(np.float64))
    # 1-D state: squeezed outputs, like the reference's expand_dims handling
    dm.disturb_estimators = None
    n1, s1, t1 = dm.predict_next_state(x[3], u[3], t_batch=None if t is None else t[3], use_gps=False)
    assert n1.shape == (x.shape[1],) and np.array_equal(n1.cpu().numpy(), d[nm + "_next"][3])


def test_predict_next_obs_device(golden):
    """predict_next_obs (dynamics.py:107-123) on device tensors stays on the
    device and equals the numpy path (cars: bit-exact; unicycle: the device
    cos/sin within 1e-15)."""
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import UnicycleEnv
    d = golden("dynamics")
    dm = DynamicsModel(UnicycleEnv(), types.SimpleNamespace(cuda=True))
    x = torch.as_tensor(d["uni_state_np"], device="cuda")
    u = torch.as_tensor(d["uni_u"], device="cuda")
    o = dm.predict_next_obs(x, u)
    ref = dm.predict_next_obs(d["uni_state_np"], d["uni_u"])
    assert o.is_cuda and o.shape == ref.shape
    assert np.max(np.abs(o.cpu().numpy() - ref)) <= 1e-15


def test_predict_next_state_device_edge_cases():
    """Cars rows without t are refused (the model prior needs t, as the
    reference's numpy path fails without it); an empty batch is a no-op."""
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import SimulatedCarsEnv
    dm = DynamicsModel(SimulatedCarsEnv(), types.SimpleNamespace(cuda=True))
    x = torch.zeros(4, 10, dtype=torch.float64, device="cuda")
    u = torch.zeros(4, 1, dtype=torch.float64, device="cuda")
    with pytest.raises(Exception):
        dm.predict_next_state(x, u, t_batch=None, use_gps=False)
    nx, sd, nt = dm.predict_next_state(x[:0], u[:0], t_batch=torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert nx.shape == (0, 10) and sd.shape == (0, 10) and nt.shape == (0,)


def test_predict_next_state_staged_rows_ragged_and_unaligned():
    """The cars kernel stages its 80-B rows through LDS (16-B accesses when
    the block's rows start 16-B aligned, element accesses otherwise): a
    ragged batch (B = 777: three full workgroups and a partial one) from an
    aligned buffer and from a view 8 bytes into one (the unaligned path)
    gives the same values bit for bit, the numpy path's within the device
    fp64 sin's ulps (car 0's v_des = 30 - 10 sin(0.2 t); random t here, the
    golden rows of test_predict_next_state_device_vs_reference are
    bit-exact), with the GP mean / std rows too."""
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import SimulatedCarsEnv
    dm = DynamicsModel(SimulatedCarsEnv(), types.SimpleNamespace(cuda=True))
    rng = np.random.default_rng(5)
    B = 777
    st = np.tile(np.array([34.0, 30.0, 28.0, 30.0, 22.0, 30.0, 16.0, 35.0, 10.0, 30.0]), (B, 1)) + rng.normal(0, 1, (B, 10))
    u = rng.uniform(-1, 1, (B, 1))
    t = np.round(rng.uniform(0, 6, B) / 0.02) * 0.02
    ref_nx, ref_sd, _ = dm.predict_next_state(st, u, t_batch=t, use_gps=False)
    ud, td = torch.as_tensor(u, device="cuda"), torch.as_tensor(t, device="cuda")
    buf = torch.zeros(B * 10 + 1, dtype=torch.float64, device="cuda")
    outs = []
    for x in (torch.as_tensor(st, device="cuda"), buf[1:].view(B, 10)):
        x.copy_(torch.as_tensor(st, device="cuda"))
        assert (x.data_ptr() % 16 == 0) == (x.storage_offset() == 0)
        nx, sd, nt = dm.predict_next_state(x, ud, t_batch=td, use_gps=False)
        assert np.max(np.abs(nx.cpu().numpy() - ref_nx)) <= 1e-13 * np.max(np.abs(ref_nx))
        assert not sd.cpu().numpy().any() and np.array_equal(nt.cpu().numpy(), t + 0.02)
        outs.append(nx.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    m32 = rng.normal(0, 0.05, (B, 10)).astype(np.float32)
    s32 = rng.uniform(0.01, 0.3, (B, 10)).astype(np.float32)

    class _GP:
        def predict(self, xq):
            return torch.as_tensor(m32, device=xq.device), torch.as_tensor(s32, device=xq.device)
    dm.disturb_estimators = _GP()
    nx, sd, _ = dm.predict_next_state(buf[1:].view(B, 10), ud, t_batch=td, use_gps=True)
    assert np.array_equal(nx.cpu().numpy(), outs[0] + 0.02 * m32.astype(np.float64))
    assert np.array_equal(sd.cpu().numpy(), 0.02 * s32.astype(np.float64))


# ----------------------------------------------------------------------------
# rcbf_model_step: every in-kernel draw against the oracle's keyed draw, and
# the output branches against oracle.model_rollout_step
# ----------------------------------------------------------------------------
DRAW_TOL = 2e-5                 # hardware fp32 log2 / cos / sin against numpy's: test_model_step_draw_moments_tails_and_key
DRAW_B = 65536 + 77             # a ragged last workgroup
DRAW_SEED = (7 << 32) | 11      # the key's high word is live
CARS_X0 = np.array([34.0, 30.0, 28.0, 30.0, 22.0, 30.0, 16.0, 35.0, 10.0, 30.0])


def _cars_rows(rng, B):
    obs = np.tile(CARS_X0, (B, 1)) + rng.normal(0, 1, (B, 10))
    obs[:, ::2] /= 100.0
    obs[:, 1::2] /= 30.0
    return obs, rng.uniform(-1, 1, (B, 1))


def _uni_rows(rng, B, heading=np.pi):
    x = np.stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-heading, heading, B)], 1)
    return O.uni_obs(x), rng.uniform(-1, 1, (B, 2))


def _cars_draws(env, obs, act, t, base, seed, counter):
    """The ten N(0, 1) draws of every row, recovered from next_obs: std = 1,
    no mean, so next_obs_k = base_k + 0.02 z_k / (100 | 30) (exact to 5e-13)."""
    from rcbf_amd.generate_rollouts import model_step
    B = obs.shape[0]
    n, *_ = model_step(env, obs, act, t, std=np.ones((B, 10), np.float32), z=None, seed=seed, counter=counter)
    return (n - base).cpu().numpy() * np.where(np.arange(10) % 2, 30.0, 100.0) / 0.02


def test_model_step_cars_draws_equal_the_keyed_oracle_draw():
    """Cars: three Philox calls (q = 0, 1, 2) for ten components, where the
    unicycle tests pin one call and two components.  Every row, every
    component, four counters, a seed above 2^32: the draws equal
    oracle.model_step_normal to 2e-5; a seed that differs in the high word
    alone gives other draws; the pooled sample is standard normal; and the 45
    correlations between components are below 6 / sqrt(n) -- two calls that
    shared a Philox block (q dropped from the counter) would repeat components
    0-3 as 4-7 and 8-9, correlation 1."""
    from rcbf_amd.generate_rollouts import model_step
    rng = np.random.default_rng(8)
    B = DRAW_B
    env = _env("SimulatedCars")
    obs, act = _cars_rows(rng, B)
    t = np.round(rng.uniform(0, 5, B) / 0.02) * 0.02
    base, *_ = model_step(env, obs, act, t, std=np.ones((B, 10), np.float32), z=np.zeros((B, 10)))
    zs, worst = [], 0.0
    for counter in range(4):
        z = _cars_draws(env, obs, act, t, base, DRAW_SEED, counter)
        want = O.model_step_normal(DRAW_SEED, np.arange(B), counter, 10)
        diff = np.abs(z - want).max(0)
        worst = max(worst, float(diff.max()))
        print(f"cars draws, counter {counter}: largest |z - oracle| per component {diff}")
        assert diff.max() <= DRAW_TOL, (counter, diff)
        zs.append(z)
    print(f"cars draws: largest |z - oracle| over {4 * B} rows x 10 components: {worst:.3g} (bar {DRAW_TOL})")
    other = (8 << 32) | 11  # the low word and everything else the same
    z2 = _cars_draws(env, obs, act, t, base, other, 0)
    assert np.abs(z2 - O.model_step_normal(other, np.arange(B), 0, 10)).max() <= DRAW_TOL
    assert np.mean(np.abs(z2 - zs[0])) > 1.0  # independent N(0, 1): E |a - b| = 2 / sqrt(pi) = 1.128
    zs = np.concatenate(zs)
    _assert_standard_normal(O.normal_moments(zs), zs.size)
    corr = np.corrcoef(zs.T)
    off = np.abs(corr[~np.eye(10, dtype=bool)])
    assert off.size == 90 and off.max() < 6.0 / np.sqrt(zs.shape[0]), off.max()


def test_model_step_unicycle_heading_draw_equals_the_keyed_oracle_draw():
    """Component 2 of the unicycle's one Philox call, recovered as the
    difference of the headings atan2(sin, cos) of next_obs (start headings in
    (-3, 3): with |dt u| <= 0.02 and |dt sd z| <= 0.024 nothing wraps), and
    components 0 and 1 under the same seed above 2^32."""
    from rcbf_amd.generate_rollouts import model_step
    rng = np.random.default_rng(9)
    B = DRAW_B
    env = _env("Unicycle")
    obs, act = _uni_rows(rng, B, heading=3.0)
    base, *_ = model_step(env, obs, act, z=np.zeros((B, 3)))
    base = base.cpu().numpy()
    worst = 0.0
    for counter in range(4):
        n, *_ = model_step(env, obs, act, z=None, seed=DRAW_SEED, counter=counter)
        n = n.cpu().numpy()
        z = np.stack([n[:, 0] - base[:, 0], n[:, 1] - base[:, 1],
                      np.arctan2(n[:, 3], n[:, 2]) - np.arctan2(base[:, 3], base[:, 2])], 1) / (0.02 * 0.2)
        diff = np.abs(z - O.model_step_normal(DRAW_SEED, np.arange(B), counter, 3)).max(0)
        worst = max(worst, float(diff.max()))
        assert diff.max() <= DRAW_TOL, (counter, diff)
    print(f"unicycle draws: largest |z - oracle| over {4 * B} rows x 3 components: {worst:.3g} (bar {DRAW_TOL})")


def _against_the_oracle(mode, obs, act, t, z, mean=None, std=None):
    """One launch against oracle.model_rollout_step at the file's bars; returns
    the oracle's outputs and the largest differences seen."""
    from rcbf_amd.generate_rollouts import model_step
    nobs, r, mask, nt = (v.cpu().numpy() for v in model_step(_env(mode), obs, act, t, mean=mean, std=std, z=z))
    on, orr, om, ot = O.model_rollout_step(mode, obs, act, t, z, mean=mean, std=std)
    d_obs, d_r = float(np.max(np.abs(nobs - on))), float(np.max(np.abs(r - orr)))
    print(f"{mode} B = {obs.shape[0]}: next_obs {d_obs:.3g}, reward {d_r:.3g} (bar 1e-12)")
    assert d_obs <= 1e-12 and d_r <= 1e-12
    assert np.array_equal(mask, om) and np.array_equal(nt, ot)
    return (on, orr, om, ot), (nobs, r, mask, nt)


def _gp_rows(rng, B, n_s):
    return rng.normal(0, 0.1, (B, n_s)).astype(np.float32), rng.uniform(0.01, 0.3, (B, n_s)).astype(np.float32)


def test_model_step_unicycle_around_the_goal():
    """Rows that end within 0.1 of the goal radius, inside and outside it: the
    goal branch (mask 0, the bonus added twice) with the prior and with GP
    mean / std rows."""
    rng = np.random.default_rng(0)
    B = 777
    r, a = rng.uniform(0.2, 0.4, B), rng.uniform(-np.pi, np.pi, B)
    x = np.stack([2.5 - r * np.cos(a), 2.5 - r * np.sin(a), rng.uniform(-np.pi, np.pi, B)], 1)
    obs, act = O.uni_obs(x), rng.uniform(-1, 1, (B, 2))
    z = rng.normal(0, 1, (B, 3))
    for mean, std in ((None, None), _gp_rows(rng, B, 3)):
        (on, orr, om, ot), (nobs, rew, mask, nt) = _against_the_oracle("Unicycle", obs, act, None, z, mean, std)
        g = np.array([2.5, 2.5]) - on[:, :2]
        d = np.linalg.norm(g, axis=1)  # the oracle's own d
        print(f"  min |d - 0.3| = {np.abs(d - 0.3).min():.3g}, {int((d <= 0.3).sum())} of {B} rows reach the goal")
        assert np.abs(d - 0.3).min() > 1e-9  # no row whose branch a last-bit difference in d could flip
        goal = d <= 0.3
        assert goal.sum() >= 100 and (~goal).sum() >= 100
        assert np.array_equal(mask, np.where(goal, 0.0, 1.0))
        shaped = -np.log(obs[:, -1]) - d
        assert np.max(np.abs(rew[goal] - shaped[goal] - 2.0)) <= 1e-12  # the bonus, twice
        assert np.max(np.abs(rew[~goal] - shaped[~goal])) <= 1e-12
        assert np.array_equal(nt, np.full(B, 0.02))


def test_model_step_cars_mask_at_the_time_limit():
    """t as the replay packer stores it (k * 0.02) and as k additions of 0.02,
    k = 295 .. 301: the two differ in their last bits, and at k = 299 on the
    two sides of the limit -- 299 * 0.02 + 0.02 >= 6.0, the 299-fold sum + 0.02
    is not.  Kernel and oracle agree on every row, with the prior and with GP
    mean / std rows (which no other test gives the cars in this kernel)."""
    rng = np.random.default_rng(1)
    B = 777
    obs, act = _cars_rows(rng, B)
    k = 295 + np.arange(B) % 7
    summed = np.zeros(302)
    for n in range(1, 302):
        summed[n] = summed[n - 1] + 0.02
    as_sum = (np.arange(B) // 7) % 2 == 1
    t = np.where(as_sum, summed[k], k * 0.02)
    assert np.any(summed[295:302] != np.arange(295, 302) * 0.02)
    assert 299 * 0.02 + 0.02 >= 6.0 and not summed[299] + 0.02 >= 6.0
    z = rng.normal(0, 1, (B, 10))
    for mean, std in ((None, None), _gp_rows(rng, B, 10)):
        (on, orr, om, ot), _ = _against_the_oracle("SimulatedCars", obs, act, t, z, mean, std)
        assert om[(k == 299) & ~as_sum].max() == 0.0 and om[(k == 299) & as_sum].min() == 1.0
        assert om[k <= 298].min() == 1.0 and om[k >= 300].max() == 0.0
        assert (om == 0.0).sum() >= 100 and (om == 1.0).sum() >= 100


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
@pytest.mark.parametrize("B", [1, 257])
def test_model_step_small_and_ragged_batches(mode, B):
    rng = np.random.default_rng(10 + B)
    cars = mode == "SimulatedCars"
    obs, act = _cars_rows(rng, B) if cars else _uni_rows(rng, B)
    t = np.round(rng.uniform(0, 6, B) / 0.02) * 0.02
    n_s = 10 if cars else 3
    _against_the_oracle(mode, obs, act, t, rng.normal(0, 1, (B, n_s)))
    _against_the_oracle(mode, obs, act, t, rng.normal(0, 1, (B, n_s)), *_gp_rows(rng, B, n_s))


@pytest.mark.parametrize("mode", ["SimulatedCars", "Unicycle"])
def test_model_step_null_next_t(mode):
    """The C ABI with next_t = NULL: rc == 0, and next_obs, reward and mask are
    bit-equal to the call that passes it; nothing is written past them."""
    import ctypes

    from rcbf_amd import _lib
    from rcbf_amd.params import make_params
    rng = np.random.default_rng(12)
    B, sent = 257, -4321.25
    cars = mode == "SimulatedCars"
    obs, act = _cars_rows(rng, B) if cars else _uni_rows(rng, B)
    dev = torch.device("cuda", 0)
    obs, act = torch.tensor(obs, device=dev), torch.tensor(act, device=dev)
    t = torch.tensor(np.round(rng.uniform(0, 6, B) / 0.02) * 0.02, device=dev)
    prm = make_params(_env(mode), 1.0)
    outs = []
    for with_t in (True, False):
        nobs = torch.full((B + 1, obs.shape[1]), sent, dtype=torch.float64, device=dev)
        rew, mask, nt = (torch.full((B + 1,), sent, dtype=torch.float64, device=dev) for _ in range(3))
        rc = _lib.load().rcbf_model_step(ctypes.byref(prm), B, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(t), None, None,
                                         None, 5, 3, _lib.ptr(nobs), _lib.ptr(rew), _lib.ptr(mask),
                                         _lib.ptr(nt if with_t else None), _lib.stream_of(dev))
        assert rc == 0
        torch.cuda.synchronize()
        assert all(v[B:].eq(sent).all() and not v[:B].eq(sent).any() for v in (nobs, rew, mask))
        outs.append((nobs, rew, mask))
        if with_t:
            assert torch.equal(nt[:B], t + 0.02) and nt[B].item() == sent
        else:
            assert bool(nt.eq(sent).all())
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(*outs))
