"""CPU-side checks of the SAC target (ABI 13, new symbols only): the fp64 port
(tests/_critic_port.py), the oracle of the GPU tests, reproduces the reference's
recorded outputs (tests/golden/td_target.npz) stage by stage;
rcbf_policy_sample / rcbf_critic_packed_floats / rcbf_critic_q /
rcbf_critic_td_target exist, document their layout and formula and reject bad
arguments before any launch; DeviceCritic packs a module into that layout and,
like sac_cbf.td_target, checks its arguments before the library is loaded; the
kernels, as they stand in librcbf_hip.so, use no scratch and spill nothing.
None of it needs a GPU."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import _critic_port as CP
import _policy_port as PP
from oracle import oracle as O
from test_abi_cpu import ROOT
from test_abi_traj_gp_cpu import _gfx950_code_objects

E_BAD_MODE, E_BAD_SHAPE, E_NULL = 1001, 1002, 1003
LIB = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_hip.so")
MODES = {"cars": "SimulatedCars", "unicycle": "Unicycle"}


def td_case(golden, env):
    g = golden("td_target")
    psd = {k[len(env) + 5:]: v for k, v in g.items() if k.startswith(env + "_psd_")}
    csd = {k[len(env) + 5:]: v for k, v in g.items() if k.startswith(env + "_csd_")}
    return psd, csd, g[env + "_action_scale"], g[env + "_action_bias"], {k[len(env) + 1:]: v for k, v in g.items()
                                                                         if k.startswith(env + "_")}, g


def oracle_safe(env, g, obs, u32):
    mode = MODES[env]
    mu, sg = O.predict_disturbance_prior(mode, obs.shape[0])
    fin, aux = O.safe_action_diff(mode, O.get_state_f32(mode, obs), np.asarray(u32, np.float32), mu.astype(np.float32),
                                  sg.astype(np.float32), float(g["gamma_b"]), hazards=g.get("unicycle_hazards")
                                  if env == "unicycle" else None)
    assert (aux["status"] == 0).all()
    return fin


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_port_reproduces_the_reference_outputs(golden, env):
    """Every recorded stage against the port on the stage's recorded inputs, within the reference's own fp32
    rounding: the allowance of a stage is 8 x (torch CPU fp32 restatement vs port) + 1e-7 max|value| -- the
    recorded values ARE a torch CPU fp32 evaluation, of the same expressions, so they err like the restatement."""
    psd, csd, scale, bias, d, g = td_case(golden, env)
    n_o, n_u = PP.ENV_SHAPES[env]
    obs, eps = d["obs"], d["eps"]
    assert obs.shape == (130, n_o) and eps.shape == (130, n_u) and csd["linear4.weight"].shape == (64, n_o + n_u)
    act, lp, mean, pre = CP.sample(psd, scale, bias, obs, eps)
    t_act, t_lp, t_mean = CP.torch_sample(psd, scale, bias, obs, eps)
    CP.check(env + " action", d["action"], t_act, act)
    CP.check(env + " mean", d["mean"], t_mean, mean)
    CP.check_log_pi(env, d["log_prob"][:, 0], t_lp, lp, pre, PP.forward(psd, obs)[1])
    q1, q2 = CP.q_forward(csd, obs, d["safe"])
    t_q1, t_q2 = CP.torch_q(csd, obs, d["safe"])
    CP.check(env + " q1", d["q1"][:, 0], t_q1, q1)
    CP.check(env + " q2", d["q2"][:, 0], t_q2, q2)
    alpha, gamma = float(g["alpha"]), float(g["gamma"])
    y = CP.target(d["reward"], d["mask"], gamma, q1, q2, alpha, d["log_prob"])
    t_y = CP.torch_target(csd, obs, d["safe"], d["reward"], d["mask"], gamma, alpha, d["log_prob"])
    CP.check(env + " next_q", d["next_q"][:, 0], t_y, y)
    # the oracle's safe action on the recorded action is the recorded safe action (the existing 1e-5)
    fin = oracle_safe(env, g, obs, d["action"])
    assert np.max(np.abs(fin - d["safe"]) / np.maximum(1, np.abs(d["safe"]))) <= 1e-5
    # the fixture exercises what it says
    raw_ls = PP.forward(psd, obs)[1]
    assert (raw_ls == 2.0).any() and (raw_ls == -20.0).any()
    assert (np.abs(pre) > 9.5).any() and (np.abs(pre) < 1).any()
    assert (d["q1"] < d["q2"]).any() and (d["q2"] < d["q1"]).any()
    assert set(np.unique(d["mask"])) == {0.0, 1.0} and alpha == 0.2 and gamma == 0.99


def test_symbols_header_and_abi_version():
    from rcbf_amd import _lib
    lib = _lib.load()
    for name in ("rcbf_policy_sample", "rcbf_critic_packed_floats", "rcbf_critic_q", "rcbf_critic_td_target"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.rcbf_abi_version() == 13 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    assert re.search(r"#define\s+RCBF_ABI_VERSION\s+13\b", hdr)
    assert re.search(r"^int64_t\s+rcbf_critic_packed_floats\s*\(", hdr, re.M)
    for name in ("rcbf_policy_sample", "rcbf_critic_q", "rcbf_critic_td_target"):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
    for word in ("model.py:94-106", "model.py:34-61", "sac_cbf.py:130-136", "2 (H (K1 + H + 3) + 4)", "w3", "b3",
                 "- 0.5 log(2 pi)) - log(scale_c (1 - y_c^2) + 1e-6)", "-0.5 z_c^2 - log_std_c", "c ascending",
                 "(x_t - mean)^2 / (2 var)", "cancellation",
                 "y = reward + (mask * gamma) * (min(q1, q2) - alpha * log_pi)", "alpha_dev"):
        assert word in hdr, word
    import rcbf_amd
    from rcbf_amd.critic import DeviceCritic
    from rcbf_amd.sac_cbf import td_target
    assert rcbf_amd.DeviceCritic is DeviceCritic and callable(td_target)
    assert callable(rcbf_amd.DevicePolicy.sample)


def test_packed_floats_follows_the_header_formula():
    from rcbf_amd import _lib
    from rcbf_amd.critic import packed_floats
    lib = _lib.load()
    for H in (32, 64, 256):
        for n_o, n_u in ((10, 1), (7, 2), (1, 1), (16, 2)):
            k1 = (n_o + n_u + 1) // 2 * 2
            want = 2 * (H * (k1 + H + 3) + 4)
            assert lib.rcbf_critic_packed_floats(n_o, n_u, H) == want == packed_floats(n_o, n_u, H)
            assert want % 8 == 0  # each net starts 16-byte aligned
    for bad in ((10, 1, 48), (10, 1, 288), (10, 3, 64), (0, 1, 64), (17, 1, 64), (10, 0, 64), (10, 1, 0)):
        assert lib.rcbf_critic_packed_floats(*bad) == -1, bad


def _host_block():
    buf = (ctypes.c_float * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15  # aligned host memory: never dereferenced, no launch is reached
    return buf, lambda off: ctypes.c_void_p(base + off)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from rcbf_amd import _lib
    lib = _lib.load()
    buf, at = _host_block()
    shapes = ({"H": 48}, {"H": 288}, {"H": 0}, {"n_u": 3}, {"n_u": 0}, {"n_o": 0}, {"n_o": 17}, {"B": -1}, {"B": 1 << 31})

    def sample(packed=at(0), n_o=10, n_u=1, H=64, B=4, obs=at(0), u=at(0), log_pi=at(0), u_mean=at(0), z=None,
               env_offset=0, has_log_std=1):
        return lib.rcbf_policy_sample(packed, n_o, n_u, H, B, obs, u, log_pi, u_mean, z, 0, 0, env_offset, has_log_std,
                                      None)

    for kw in shapes + ({"env_offset": -1},):
        assert sample(**kw) == E_BAD_SHAPE, kw
    assert sample(has_log_std=0) == E_BAD_MODE
    for f in ("packed", "obs", "u"):
        assert sample(**{f: None}) == E_NULL, f
    for off in (4, 8, 12):
        assert sample(packed=at(off)) == E_BAD_SHAPE, off
    for f in ("obs", "u", "log_pi", "u_mean", "z"):
        assert sample(**{f: at(2)}) == E_BAD_SHAPE, f
    assert sample(B=0) == 0 and sample(B=0, packed=None, obs=None, u=None) == 0 and sample(B=0, H=48) == E_BAD_SHAPE

    def q(packed=at(0), n_o=10, n_u=1, H=64, B=4, obs=at(0), act=at(0), q1=at(0), q2=at(0)):
        return lib.rcbf_critic_q(packed, n_o, n_u, H, B, obs, act, q1, q2, None)

    def td(packed=at(0), n_o=10, n_u=1, H=64, B=4, obs=at(0), act=at(0), reward=at(0), mask=at(0), log_pi=at(0),
           alpha_dev=None, y=at(0), q1=None, q2=None):
        return lib.rcbf_critic_td_target(packed, n_o, n_u, H, B, obs, act, reward, mask, log_pi, 0.2, alpha_dev, 0.99, y,
                                         q1, q2, None)

    for call, required, optional in ((q, ("packed", "obs", "act", "q1", "q2"), ()),
                                     (td, ("packed", "obs", "act", "reward", "mask", "log_pi", "y"),
                                      ("alpha_dev", "q1", "q2"))):
        for kw in shapes:
            assert call(**kw) == E_BAD_SHAPE, (call.__name__, kw)
        for f in required:
            assert call(**{f: None}) == E_NULL, (call.__name__, f)
        for off in (4, 8, 12):
            assert call(packed=at(off)) == E_BAD_SHAPE, off
        for f in required[1:] + optional:
            assert call(**{f: at(2)}) == E_BAD_SHAPE, (call.__name__, f)
        assert call(B=0) == 0 and call(B=0, **{f: None for f in required}) == 0 and call(B=0, H=48) == E_BAD_SHAPE


def test_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    import yaml
    found = {}
    for k, blob in enumerate(_gfx950_code_objects(LIB)):
        if b"k_critic_q" not in blob and b"k_actor_sample" not in blob:
            continue
        co = tmp_path / f"co{k}.elf"
        co.write_bytes(blob)
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(co)], check=True,
                             capture_output=True, text=True).stdout
        m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
        assert m, "no AMDGPU metadata"
        for kern in yaml.safe_load(m.group(1))["amdhsa.kernels"]:
            if "k_critic_q" in kern[".name"] or "k_actor_sample" in kern[".name"]:
                found[kern[".name"]] = kern
    assert len(found) == 6, sorted(found)  # sample x {32, 64 rows}; {q, td target} x {32, 64 rows}
    for name, kern in found.items():
        assert "k_policy_act" not in name
        assert kern[".private_segment_fixed_size"] == 0, name
        assert kern[".sgpr_spill_count"] == 0 and kern[".vgpr_spill_count"] == 0, name
        assert kern[".max_flat_workgroup_size"] == 256, name


def test_device_critic_packs_the_header_layout():
    """On host tensors (packing is torch ops): every weight lands where the header says, for both nets."""
    import torch

    from rcbf_amd.critic import DeviceCritic, packed_floats
    for (n_o, n_u), H in (((10, 1), 64), ((7, 2), 32), ((16, 2), 256), ((1, 1), 32)):
        n_in = n_o + n_u
        sd = CP.seeded_critic(n_in, H, 11)
        m = CP.torch_critic(sd)
        crit = DeviceCritic(m, device="cpu")
        p = crit.packed.numpy()
        assert p.size == packed_floats(n_o, n_u, H) and crit.packed.data_ptr() % 16 == 0
        k1 = (n_in + 1) // 2 * 2
        net = H * (k1 + H + 3) + 4
        for j, (a, b, c) in enumerate(((1, 2, 3), (4, 5, 6))):
            q = p[j * net:(j + 1) * net]
            w1p = q[:H * k1].reshape(H // 32, k1 // 2, 64)
            w2p = q[H * k1 + H:H * k1 + H + H * H].reshape(H // 32, H // 8, 64, 4)
            w1 = np.zeros((H, k1), np.float32)
            w1[:, :n_in] = sd[f"linear{a}.weight"]
            for cb, s, l in ((0, 0, 0), (H // 32 - 1, k1 // 2 - 1, 63), (0, k1 // 2 - 1, 37), (H // 64, 0, 5)):
                assert w1p[cb, s, l] == w1[32 * cb + (l & 31), 2 * s + (l >> 5)]
            for cb, s4, l, jj in ((0, 0, 0, 0), (H // 32 - 1, H // 8 - 1, 63, 3), (0, 1, 37, 2), (H // 64, 3, 5, 1)):
                assert w2p[cb, s4, l, jj] == sd[f"linear{b}.weight"][32 * cb + (l & 31), 2 * (4 * s4 + jj) + (l >> 5)]
            off = H * k1
            assert np.array_equal(q[off:off + H], sd[f"linear{a}.bias"])
            off += H + H * H
            assert np.array_equal(q[off:off + H], sd[f"linear{b}.bias"])
            off += H
            assert np.array_equal(q[off:off + H], sd[f"linear{c}.weight"][0])
            off += H
            assert q[off] == sd[f"linear{c}.bias"][0] and not q[off + 1:off + 4].any() and off + 4 == net
        ptr = crit.packed.data_ptr()
        with torch.no_grad():
            m.linear6.bias.add_(1.0)
        crit.refresh()
        assert crit.packed.data_ptr() == ptr and crit.packed.numpy()[-4] == sd["linear6.bias"][0] + np.float32(1.0)


def test_device_critic_and_td_target_check_before_any_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.critic import DeviceCritic
    from rcbf_amd.policy import DevicePolicy
    from rcbf_amd.sac_cbf import td_target

    def no_library():
        raise AssertionError("reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    m = CP.torch_critic(CP.seeded_critic(11, 64, 0))
    crit = DeviceCritic(m, device="cpu")  # host tensors stand in: every check fails before a launch
    obs, act, col = torch.zeros(5, 10), torch.zeros(5, 1), torch.zeros(5, 1)
    for o, a in ((torch.zeros(5, 9), act), (obs, torch.zeros(5, 2)), (obs, torch.zeros(4, 1)), (obs, torch.zeros(5, 3)),
                 (obs.double(), act), (obs, act.double()), (np.zeros((5, 10), np.float32), act), (torch.zeros(10, 5).t(), act),
                 (obs, torch.zeros(5))):
        with pytest.raises(ValueError):
            crit.q(o, a)
        with pytest.raises(ValueError):
            crit.td_target(o, a, col, col, col, 0.2, 0.99)
    with pytest.raises(ValueError):
        crit.q(obs, act, out=(torch.zeros(4, 1), torch.zeros(5, 1)))
    with pytest.raises(ValueError):
        crit.q(obs, act, out=torch.zeros(5, 2))
    for kw in ({"reward": torch.zeros(4, 1)}, {"mask": torch.zeros(5, 2)}, {"log_pi": col.double()}, {"out": torch.zeros(4, 1)},
               {"alpha": torch.zeros(2)}, {"alpha": torch.zeros(1, dtype=torch.float64)}, {"q_out": (col,)},
               {"q_out": (torch.zeros(4, 1), col)}):
        args = {"reward": col, "mask": col, "log_pi": col, "alpha": 0.2, "gamma": 0.99, **kw}
        with pytest.raises(ValueError):
            crit.td_target(obs, act, **args)
    with pytest.raises(ValueError, match="HIP device"):
        crit.q(obs, act)  # well-formed host tensors: still no library call
    with pytest.raises(ValueError, match="HIP device"):
        crit.td_target(obs, act, col, torch.zeros(5), col, torch.tensor(0.2), 0.99)
    # modules the kernel does not take
    for n_in, H in ((11, 48), (19, 64), (1, 64), (11, 288)):
        with pytest.raises(ValueError):
            DeviceCritic(CP.torch_critic(CP.seeded_critic(n_in, H, 0)), device="cpu")
    with pytest.raises(ValueError):
        DeviceCritic(types.SimpleNamespace(linear1=m.linear1, linear2=m.linear2, linear3=m.linear3), device="cpu")
    bad = CP.torch_critic(CP.seeded_critic(11, 64, 0))
    bad.linear5 = torch.nn.Linear(32, 64)
    with pytest.raises(ValueError):
        DeviceCritic(bad, device="cpu")
    # DevicePolicy.sample and the whole block
    pol = DevicePolicy(PP.torch_module(PP.seeded_weights(10, 1, 64, 3), np.ones(1), np.zeros(1)), device="cpu")
    for kw in ({"z": torch.zeros(5, 2)}, {"z": torch.zeros(4, 1)}, {"out": (act, col)}, {"out": (act, torch.zeros(5, 2), act)},
               {"out": (torch.zeros(4, 1), col, act)}):
        with pytest.raises(ValueError):
            pol.sample(obs, **kw)
    with pytest.raises(ValueError):
        pol.sample(torch.zeros(5, 9))
    with pytest.raises(ValueError, match="HIP device"):
        pol.sample(obs)
    det = PP.torch_module(PP.seeded_weights(10, 1, 64, 3), np.ones(1), np.zeros(1))
    del det.log_std_linear
    with pytest.raises(NotImplementedError):
        DevicePolicy(det, device="cpu").sample(obs)
    for o, r, k in ((torch.zeros(5, 9), col, col), (obs, torch.zeros(4), col), (obs, col, torch.zeros(6, 1)), (torch.zeros(10), col, col)):
        with pytest.raises(ValueError):
            td_target(pol, crit, None, None, o, r, k, 0.2, 0.99)
    with pytest.raises(ValueError, match="HIP device"):  # strided fp64 views are converted, then sample refuses the host
        td_target(pol, crit, None, None, torch.zeros(10, 5, dtype=torch.float64).t(), torch.zeros(5, dtype=torch.float64),
                  torch.zeros(5, dtype=torch.float64), 0.2, 0.99)
