"""CPU-side checks of the policy forward (ABI 13, new symbols only): the fp64
port (tests/_policy_port.py), the oracle of the GPU tests, reproduces the
reference's recorded outputs (tests/golden/policy.npz); rcbf_policy_act /
rcbf_policy_packed_floats exist, document their layout and reject bad
arguments before any launch; DevicePolicy packs a module into that layout and,
like evaluate_policy, checks its arguments before the library is loaded; the
kernel, as it stands in librcbf_hip.so, uses no scratch and spills nothing.
None of it needs a GPU."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import _policy_port as PP
from test_abi_cpu import ROOT
from test_abi_traj_gp_cpu import _gfx950_code_objects

E_BAD_MODE, E_BAD_SHAPE, E_NULL = 1001, 1002, 1003
LIB = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_hip.so")


def golden_case(golden, env):
    g = golden("policy")
    sd = {k[len(env) + 4:]: v for k, v in g.items() if k.startswith(env + "_sd_")}
    return sd, g[env + "_action_scale"], g[env + "_action_bias"], g


@pytest.mark.parametrize("env", ["cars", "unicycle"])
def test_port_reproduces_the_reference_outputs(golden, env):
    """port fp64 vs the reference's torch CPU fp32.  The action: <= 2e-6 abs on all 130 rows.  mean and
    log_std: <= 2e-6 abs on the 65 real rows.  The other 65 are those rows x20: the network is piecewise
    linear with small biases, so every pre-activation, and with it torch's fp32 rounding error, is x20 too
    (recorded values reach 10 .. 45, where ONE fp32 ulp is 1e-6 .. 4e-6; torch's sums are 2.5e-6 .. 2e-5 off
    the exact value on each of 400 seeds tried): the same bound at the rows' scale, 20 x 2e-6."""
    sd, scale, bias, g = golden_case(golden, env)
    obs = g[env + "_obs"]
    n_o, n_u = PP.ENV_SHAPES[env]
    assert obs.shape == (130, n_o) and sd["linear1.weight"].shape == (64, n_o) and scale.shape == (n_u,)
    mean, ls = PP.forward(sd, obs)
    for got, key in ((mean, "_mean"), (ls, "_log_std")):
        err = np.abs(got - g[env + key])
        print(env, key, "real rows", err[:65].max(), "x20 rows", err[65:].max())
        assert err[:65].max() <= 2e-6, key
        assert err[65:].max() <= 20 * 2e-6, key
    assert np.max(np.abs(PP.act(sd, scale, bias, obs) - g[env + "_action_mean"])) <= 2e-6
    # the fixture exercises what it says: both clamps, saturated and unsaturated tanh
    assert (g[env + "_log_std"] == 2.0).any() and (g[env + "_log_std"] == -20.0).any()
    assert (np.abs(g[env + "_action_mean"]) == scale).any() and (np.abs(g[env + "_mean"]) < 1).any()


def test_symbols_header_and_abi_version():
    from rcbf_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rcbf_policy_act") and hasattr(lib, "rcbf_policy_packed_floats")
    assert lib.rcbf_abi_version() == 13 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    assert re.search(r"#define\s+RCBF_ABI_VERSION\s+13\b", hdr)
    assert re.search(r"^int64_t\s+rcbf_policy_packed_floats\s*\(", hdr, re.M)
    assert re.search(r"^int\s+rcbf_policy_act\s*\(", hdr, re.M)
    assert "model.py:86-106" in hdr and "sac_cbf.py:72-75" in hdr
    for word in ("W1p", "W2p", "action_scale", "k ascending", "RCBF_POLICY_MEAN", "RCBF_POLICY_SAMPLE"):
        assert word in hdr, word
    import rcbf_amd
    from rcbf_amd.evaluator import evaluate_policy
    from rcbf_amd.policy import DevicePolicy
    assert rcbf_amd.DevicePolicy is DevicePolicy and rcbf_amd.evaluate_policy is evaluate_policy


def test_packed_floats_follows_the_header_formula():
    from rcbf_amd import _lib
    from rcbf_amd.policy import packed_floats
    lib = _lib.load()
    for H in (32, 64, 256):
        for n_o, n_u in ((10, 1), (7, 2), (1, 1), (16, 2)):
            k1 = n_o + (n_o & 1)
            want = H * (k1 + H + 2 + 2 * n_u) + 16
            assert lib.rcbf_policy_packed_floats(n_o, n_u, H) == want == packed_floats(n_o, n_u, H)
            assert want % 4 == 0
    for bad in ((10, 1, 48), (10, 1, 288), (10, 3, 64), (0, 1, 64), (17, 1, 64), (10, 0, 64), (10, 1, 0)):
        assert lib.rcbf_policy_packed_floats(*bad) == -1, bad


def test_policy_act_rejects_bad_arguments_without_a_gpu():
    from rcbf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15  # aligned host memory: never dereferenced, no launch is reached

    def at(off):
        return ctypes.c_void_p(base + off)

    def call(packed=at(0), n_o=10, n_u=1, H=64, B=4, obs=at(0), u=at(0), mode=0, z=None, env_offset=0):
        return lib.rcbf_policy_act(packed, n_o, n_u, H, B, obs, u, mode, z, 0, 0, env_offset, None)

    for kw in ({"H": 48}, {"H": 288}, {"H": 0}, {"n_u": 3}, {"n_u": 0}, {"n_o": 0}, {"n_o": 17}, {"B": -1},
               {"B": 1 << 31}, {"env_offset": -1}):
        assert call(**kw) == E_BAD_SHAPE, kw
    for mode in (2, -1):
        assert call(mode=mode) == E_BAD_MODE, mode
    for f in ("packed", "obs", "u"):
        assert call(**{f: None}) == E_NULL, f
    for off in (4, 8, 12):
        assert call(packed=at(off)) == E_BAD_SHAPE, off
    for f in ("obs", "u", "z"):
        assert call(mode=1, **{f: at(2)}) == E_BAD_SHAPE, f
    assert call(B=0) == 0 and call(B=0, packed=None, obs=None, u=None, mode=1) == 0  # an empty batch is a no-op
    assert call(B=0, H=48) == E_BAD_SHAPE  # ... of a valid shape


def test_kernel_uses_no_scratch_and_does_not_spill(tmp_path):
    import yaml
    found = {}
    for k, blob in enumerate(_gfx950_code_objects(LIB)):
        if b"k_policy_act" not in blob:
            continue
        co = tmp_path / f"co{k}.elf"
        co.write_bytes(blob)
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(co)], check=True,
                             capture_output=True, text=True).stdout
        m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
        assert m, "no AMDGPU metadata"
        for kern in yaml.safe_load(m.group(1))["amdhsa.kernels"]:
            if "k_policy_act" in kern[".name"]:
                found[kern[".name"]] = kern
    assert len(found) == 4, sorted(found)  # {mean, sample} x {32-row, 64-row tiles}
    for name, kern in found.items():
        assert kern[".private_segment_fixed_size"] == 0, name
        assert kern[".sgpr_spill_count"] == 0 and kern[".vgpr_spill_count"] == 0, name
        assert kern[".max_flat_workgroup_size"] == 256, name


def _module(env="cars", H=64, log_std=True, seed=3):
    n_o, n_u = PP.ENV_SHAPES[env]
    sd = PP.seeded_weights(n_o, n_u, H, seed)
    m = PP.torch_module(sd, np.full(n_u, 2.0, np.float32), np.full(n_u, 0.5, np.float32))
    if not log_std:
        del m.log_std_linear
    return sd, m


def test_device_policy_packs_the_header_layout():
    """On host tensors (packing is torch ops): every weight lands where the header says."""
    from rcbf_amd.policy import DevicePolicy, packed_floats
    for env, H in (("cars", 64), ("unicycle", 32), ("unicycle", 256)):
        sd, m = _module(env, H)
        n_o, n_u = PP.ENV_SHAPES[env]
        pol = DevicePolicy(m, device="cpu")
        p = pol.packed.numpy()
        assert p.size == packed_floats(n_o, n_u, H) and pol.packed.data_ptr() % 16 == 0
        k1 = n_o + (n_o & 1)
        w1p = p[:H * k1].reshape(H // 32, k1 // 2, 64)
        w2p = p[H * k1 + H:H * k1 + H + H * H].reshape(H // 32, H // 8, 64, 4)
        w1 = np.zeros((H, k1), np.float32)
        w1[:, :n_o] = sd["linear1.weight"]
        for cb, s, l in ((0, 0, 0), (H // 32 - 1, k1 // 2 - 1, 63), (0, 1, 37), (H // 64, 2, 5)):
            assert w1p[cb, s, l] == w1[32 * cb + (l & 31), 2 * s + (l >> 5)]
        for cb, s4, l, j in ((0, 0, 0, 0), (H // 32 - 1, H // 8 - 1, 63, 3), (0, 1, 37, 2), (H // 64, 3, 5, 1)):
            assert w2p[cb, s4, l, j] == sd["linear2.weight"][32 * cb + (l & 31), 2 * (4 * s4 + j) + (l >> 5)]
        off = H * k1
        assert np.array_equal(p[off:off + H], sd["linear1.bias"])
        off += H + H * H
        assert np.array_equal(p[off:off + H], sd["linear2.bias"])
        off += H
        assert np.array_equal(p[off:off + n_u * H], sd["mean_linear.weight"].ravel())
        off += n_u * H
        assert np.array_equal(p[off:off + n_u], sd["mean_linear.bias"])
        off += 4
        assert np.array_equal(p[off:off + n_u * H], sd["log_std_linear.weight"].ravel())
        off += n_u * H
        assert np.array_equal(p[off:off + n_u], sd["log_std_linear.bias"])
        off += 4
        assert np.array_equal(p[off:off + n_u], np.full(n_u, 2.0, np.float32))
        assert np.array_equal(p[off + 4:off + 4 + n_u], np.full(n_u, 0.5, np.float32)) and off + 8 == p.size
        # refresh() re-packs into the same buffer
        ptr = pol.packed.data_ptr()
        import torch
        with torch.no_grad():
            m.linear1.bias.add_(1.0)
        pol.refresh()
        assert pol.packed.data_ptr() == ptr and np.array_equal(pol.packed.numpy()[H * k1:H * k1 + H],
                                                                 sd["linear1.bias"] + np.float32(1.0))


def test_device_policy_checks_before_any_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.evaluator import evaluate_policy
    from rcbf_amd.policy import DevicePolicy

    def no_library():
        raise AssertionError("reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    _, m = _module("cars", 64)
    pol = DevicePolicy(m, device="cpu")  # host tensors stand in: every check fails before a launch
    obs = torch.zeros(5, 10)
    for bad in (torch.zeros(5, 9), torch.zeros(5, 10, dtype=torch.float64), torch.zeros(10), np.zeros((5, 10), np.float32),
                torch.zeros(10, 5).t()):
        with pytest.raises(ValueError):
            pol.act(bad, evaluate=True)
    for kw in ({"out": torch.zeros(4, 1)}, {"out": torch.zeros(5, 2)}, {"out": torch.zeros(5, 1, dtype=torch.float64)},
               {"z": torch.zeros(5, 2)}, {"z": torch.zeros(4, 1)}):
        with pytest.raises(ValueError):
            pol.act(obs, evaluate=False, **kw)
    with pytest.raises(ValueError):
        pol.act(obs, evaluate=True, z=torch.zeros(5, 1))
    with pytest.raises(ValueError, match="HIP device"):
        pol.act(obs, evaluate=True)  # well-formed host tensors: still no library call
    _, det = _module("cars", 64, log_std=False)
    dpol = DevicePolicy(det, device="cpu")
    assert not dpol.has_log_std
    with pytest.raises(NotImplementedError):
        dpol.act(obs, evaluate=False)
    # shapes the kernel does not take
    for n_o, n_u, H in ((10, 1, 48), (10, 3, 64), (17, 1, 64), (10, 1, 288)):
        sd = PP.seeded_weights(n_o, n_u, H, 0)
        with pytest.raises(ValueError):
            DevicePolicy(PP.torch_module(sd, np.ones(n_u), np.zeros(n_u)), device="cpu")
    with pytest.raises(ValueError):
        DevicePolicy(types.SimpleNamespace(linear1=m.linear1, linear2=m.linear2), device="cpu")
    # evaluate_policy
    env = types.SimpleNamespace(num_envs=5, max_episode_steps=300, n_o=10, n_u=1, obs=obs)
    for kw in ({"steps": 0}, {"steps": -3}):
        with pytest.raises(ValueError):
            evaluate_policy(env, pol, None, **kw)
    with pytest.raises(ValueError):
        evaluate_policy(env, object(), None)
    uni = types.SimpleNamespace(num_envs=5, max_episode_steps=1000, n_o=7, n_u=2, obs=torch.zeros(5, 7))
    with pytest.raises(ValueError):
        evaluate_policy(uni, pol, None)
    with pytest.raises(NotImplementedError):
        evaluate_policy(env, dpol, None, evaluate=False)
    with pytest.raises(ValueError, match="device env"):
        evaluate_policy(env, pol, None, steps=3)
