"""CPU-side checks of the trajectory episode statistics (ABI 13, new symbols
only): rcbf_traj_episode_stats_f64 / rcbf_traj_episode_stats_scratch_bytes
exist and reject bad arguments before any launch; the new kernels, as they
stand in librcbf_hip.so, use no scratch and spill nothing;
EpisodeStats.update checks its arguments before the library is loaded; and the
numpy port of the reference's bookkeeping (tests/_episode_port.py), the oracle
of the GPU tests, chains through its carry bit for bit.  None of it needs a
GPU."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from _episode_port import bits, episode_loop, same_records, synthetic
from test_abi_cpu import ROOT
from test_abi_traj_gp_cpu import _gfx950_code_objects

E_BAD_SHAPE, E_NULL = 1002, 1003
LIB = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_hip.so")


def test_symbols_and_abi_version():
    from rcbf_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rcbf_traj_episode_stats_f64") and hasattr(lib, "rcbf_traj_episode_stats_scratch_bytes")
    assert lib.rcbf_abi_version() == 13 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    assert re.search(r"#define\s+RCBF_ABI_VERSION\s+13\b", hdr)
    for name in ("rcbf_traj_episode_stats_f64", "rcbf_traj_episode_stats_scratch_bytes"):
        assert re.search(r"^int(64_t)?\s+%s\s*\(" % name, hdr, re.M), name
    assert "main.py:98-101" in hdr and "main.py:140-144" in hdr
    import rcbf_amd
    from rcbf_amd.episode_stats import EpisodeStats
    assert rcbf_amd.EpisodeStats is EpisodeStats


def test_scratch_bytes_is_a_count_per_step_and_wave_plus_the_total():
    from rcbf_amd import _lib
    lib = _lib.load()
    for B, K in ((1, 1), (64, 5), (65, 5), (130, 7), (65536, 20), (64, 1000)):
        assert lib.rcbf_traj_episode_stats_scratch_bytes(B, K) == 8 * ((B + 63) // 64 * K + 1)
    assert lib.rcbf_traj_episode_stats_scratch_bytes(1 << 31, 1000) == 8 * ((1 << 25) * 1000 + 1)  # past 2^32 bytes
    assert lib.rcbf_traj_episode_stats_scratch_bytes(-1, 5) == 0 == lib.rcbf_traj_episode_stats_scratch_bytes(5, 0)


def test_episode_stats_rejects_bad_arguments_without_a_gpu():
    from rcbf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15  # 16-byte aligned host memory: never dereferenced, no launch is reached

    def at(off):
        return ctypes.c_void_p(base + off)

    p = at(0)
    records = ("env", "step", "length", "ret", "cst")

    def call(env=p, step=p, length=p, ret=p, cst=p, count=p, scratch=p, B=4, K=2, P=4, reward=p, cost=p, done=p,
             carry_in=at(0), len_in=at(0), carry_out=at(1024), len_out=at(1024), auto_reset=1, max_rows=8):
        return lib.rcbf_traj_episode_stats_f64(env, step, length, ret, cst, count, scratch, B, K, P, reward, cost,
                                               done, carry_in, len_in, carry_out, len_out, auto_reset, max_rows, None)

    assert call(B=0) == 0  # an empty batch is a no-op
    assert call(B=0, reward=None, count=None) == 0
    for kw in ({"K": 0}, {"K": -1}, {"B": -1}, {"P": 3}, {"max_rows": -1}, {"B": (1 << 31), "P": (1 << 31)}):
        assert call(**kw) == E_BAD_SHAPE, kw
    for f in ("reward", "done", "count", "scratch", *records):
        assert call(**{f: None}) == E_NULL, f
    # the count-only call needs no record array: without them it gets as far as the alignment checks
    assert call(max_rows=0, count=at(4), **{f: None for f in records}) == E_BAD_SHAPE
    assert call(max_rows=0, cost=None, carry_in=None, len_in=None, carry_out=None, len_out=None, scratch=at(4),
                **{f: None for f in records}) == E_BAD_SHAPE  # ... and the nullable inputs are no null error
    # alignment: the carries are one 16-byte access per lane, 8-byte values 8, 4-byte values 4 (done: bytes)
    for f in ("carry_in", "carry_out"):
        assert call(**{f: at(1024 + 8)}) == E_BAD_SHAPE, f
    for f in ("ret", "cst", "count", "scratch"):
        assert call(**{f: at(4)}) == E_BAD_SHAPE, f
    for f in ("env", "step", "length", "reward", "cost", "len_in", "len_out"):
        assert call(**{f: at(1024 + 2)}) == E_BAD_SHAPE, f
    # in and out are separate arrays: B = 4 envs are 64 bytes of carry and 16 of lengths
    for off in (0, 16, 48):
        assert call(carry_in=at(512), carry_out=at(512 + off)) == E_BAD_SHAPE, off
        assert call(carry_out=at(512), carry_in=at(512 + off)) == E_BAD_SHAPE, off
    for off in (0, 4, 12):
        assert call(len_in=at(512), len_out=at(512 + off)) == E_BAD_SHAPE, off
        assert call(len_out=at(512), len_in=at(512 + off)) == E_BAD_SHAPE, off


def test_episode_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    import yaml
    found = {}
    for k, blob in enumerate(_gfx950_code_objects(LIB)):
        if b"k_traj_ep_pack" not in blob:
            continue
        co = tmp_path / f"co{k}.elf"
        co.write_bytes(blob)
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(co)], check=True,
                             capture_output=True, text=True).stdout
        m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
        assert m, "no AMDGPU metadata"
        for kern in yaml.safe_load(m.group(1))["amdhsa.kernels"]:
            if "k_traj_ep_" in kern[".name"]:
                found[kern[".name"]] = kern
    assert len(found) == 3, sorted(found)  # count, pack x {with cost, without}
    assert sum("k_traj_ep_count" in n for n in found) == 1 and sum("k_traj_ep_pack" in n for n in found) == 2
    for name, kern in found.items():
        assert kern[".private_segment_fixed_size"] == 0, name
        assert kern[".sgpr_spill_count"] == 0 and kern[".vgpr_spill_count"] == 0, name
        assert kern[".max_flat_workgroup_size"] == 64, name
        assert kern[".group_segment_fixed_size"] == 0, name  # plain per-lane stores: no LDS staging


def _stub_env(B=4):
    import torch
    return types.SimpleNamespace(num_envs=B, step_count=torch.zeros(B, dtype=torch.int32))


def test_update_checks_its_arguments_before_any_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.episode_stats import EpisodeStats

    def no_library():
        raise AssertionError("update reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    K, B = 3, 4
    stats = EpisodeStats(_stub_env(B), device="cpu")  # host tensors stand in: every check fails before a launch

    def traj(P=64):
        return {"reward": torch.zeros(K, P)[:, :B], "cost": torch.zeros(K, P)[:, :B],
                "done": torch.zeros(K, P, dtype=torch.uint8)[:, :B]}

    for f in ("reward", "done"):
        t = traj()
        del t[f]
        with pytest.raises(ValueError, match=f):
            stats.update(t)
    t = traj()
    del t["cost"]  # optional; host tensors are refused last
    with pytest.raises(ValueError, match="HIP device"):
        stats.update(t)
    with pytest.raises(ValueError, match="HIP device"):
        stats.update(traj())
    for f, bad in (("done", torch.zeros(K, 64, dtype=torch.int32)[:, :B]), ("done", torch.zeros(K, 64)[:, :B] != 0),
                   ("reward", torch.zeros(K, 64, dtype=torch.float64)[:, :B]),
                   ("cost", torch.zeros(K, 64, dtype=torch.float64)[:, :B]),
                   ("reward", torch.zeros(K, 64)[:, :B + 1]), ("cost", torch.zeros(K, 64, 1)[:, :B]),
                   ("reward", torch.zeros(K, B).numpy())):
        t = traj()
        t[f] = bad
        with pytest.raises(ValueError, match=f):
            stats.update(t)
    t = traj()
    t["cost"] = torch.zeros(K, 128)[:, :B]  # another pitch
    with pytest.raises(ValueError, match="pitch"):
        stats.update(t)
    t = traj()
    t["reward"] = torch.zeros(K, 2 * B)[:, ::2]  # not dense along the envs
    with pytest.raises(ValueError, match="reward"):
        stats.update(t)
    t = traj()
    t["done"] = torch.zeros(B, K, dtype=torch.uint8).t()  # env-major
    with pytest.raises(ValueError, match="done"):
        stats.update(t)
    t = traj()
    t["cost"] = torch.zeros(K - 1, 64)[:, :B]  # fewer rows than the others are asked for
    with pytest.raises(ValueError, match="cost"):
        stats.update(t, rows=K)
    with pytest.raises(ValueError, match="rows"):
        stats.update(traj(), rows=K + 1)
    with pytest.raises(ValueError, match="rows"):
        stats.update(traj(), rows=0)
    with pytest.raises(ValueError, match="max_episodes"):
        stats.update(traj(), max_episodes=-1)
    carry, length = stats.running()
    assert tuple(carry.shape) == (B, 2) and carry.dtype == torch.float64 and not carry.any()
    assert tuple(length.shape) == (B,) and length.dtype == torch.int32 and not length.any()


def test_initial_lengths_are_a_clone_of_the_env_step_count_and_reset_zeroes():
    import torch

    from rcbf_amd.episode_stats import EpisodeStats
    env = _stub_env(5)
    env.step_count += torch.arange(5, dtype=torch.int32) * 7
    stats = EpisodeStats(env, device="cpu")
    assert torch.equal(stats.running()[1], env.step_count)
    env.step_count += 1  # a clone: the env's own counter moves on alone
    assert torch.equal(stats.running()[1] + 1, env.step_count)
    stats._carry += 2.5
    stats.reset()
    assert not stats.running()[0].any() and not stats.running()[1].any()


def test_an_env_batch_of_zero_gives_no_records_and_no_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.episode_stats import EpisodeStats

    def no_library():
        raise AssertionError("an empty batch reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    stats = EpisodeStats(_stub_env(0), device="cpu")
    out = stats.update({"reward": torch.zeros(3, 64)[:, :0], "done": torch.zeros(3, 64, dtype=torch.uint8)[:, :0]})
    assert out["n_episodes"] == 0
    assert all(out[f].shape == (0,) for f in ("env", "step", "length", "reward", "cost"))
    assert out["reward"].dtype == torch.float64 and out["length"].dtype == torch.int32


@pytest.mark.parametrize("K,K1,B", [(37, 1, 5), (37, 20, 70), (12, 11, 3)])
def test_the_numpy_port_chains_through_its_carry_bit_for_bit(K, K1, B):
    """One run of K steps equals two runs of K1 + (K - K1) steps, the second
    started from the first's carry and lengths."""
    s = synthetic(K, B, seed=K * 100 + B)
    for cost in (s["cost"], None):
        whole, carry, length = episode_loop(s["reward"], cost, s["done"], s["carry"], s["len"])
        assert whole["env"].size == int(s["done"].sum()) > 0
        c1 = None if cost is None else cost[:K1]
        c2 = None if cost is None else cost[K1:]
        a, carry_a, len_a = episode_loop(s["reward"][:K1], c1, s["done"][:K1], s["carry"], s["len"])
        b, carry_b, len_b = episode_loop(s["reward"][K1:], c2, s["done"][K1:], carry_a, len_a)
        b["step"] = b["step"] + K1
        joined = {f: np.concatenate([a[f], b[f]]) for f in whole}
        assert same_records(joined, whole)
        assert np.array_equal(bits(carry_b), bits(carry)) and np.array_equal(len_b, length)
        # the order of the additions shows in these inputs: the sums added backwards differ somewhere
        # (the carry has a full fp64 mantissa: from it on the additions round)
        fwd, back = s["carry"][:, 0].copy(), s["carry"][:, 0].copy()
        for j in range(K):
            fwd, back = fwd + s["reward"][j].astype(np.float64), back + s["reward"][K - 1 - j].astype(np.float64)
        assert B < 70 or not np.array_equal(bits(back), bits(fwd))  # (among 70 envs; a handful can agree)
        if cost is None:  # the cost column is the carry's until the first reset, then zero
            assert not whole["cost"][whole["length"] <= whole["step"]].any()
