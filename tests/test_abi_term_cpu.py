"""CPU-side checks of the kernels that keep the terminal observation
(rcbf::k_safe_steps_term in csrc/rcbf_safe_step.hpp, instantiated in
csrc/rcbf_steps_term.hip) as they stand in librcbf_steps_term.co, the third code
object rcbf_aql_open loads: the argument block csrc/rcbf_aql.hip writes
(SafeStepsTermArgs = SafeStepsTrajArgs + term_obs), no hidden arguments, no
scratch, no register spill, one kernel per mode / hazard count and workgroup
size, no FLAT access, every store in the step loop and no full vmcnt wait in
it; the new bit's Python mirror; and the host-side argument checks of
rcbf_aql_safe_step_term_plan, rcbf_traj_pack_replay_f64 and
ReplayMemory.push_trajectory, none of which needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from test_abi_cpu import ROOT
from test_abi_traj_cpu import _header_defs, _loop_addresses
from test_fused_loop_isa_cpu import OBJDUMP

TERM_PREFIX = "_ZN4rcbf17k_safe_steps_termI"
TERM_CO = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_steps_term.co")
E_BAD_MODE, E_BAD_SHAPE, E_NULL = 1001, 1002, 1003


def _term_kernels():
    import yaml
    if not os.path.exists(TERM_CO):
        pytest.skip("librcbf_steps_term.co not built")
    txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", TERM_CO], check=True, capture_output=True,
                         text=True).stdout
    m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
    assert m, "no AMDGPU metadata in librcbf_steps_term.co"
    return [k for k in yaml.safe_load(m.group(1))["amdhsa.kernels"] if k[".name"].startswith(TERM_PREFIX)]


def test_term_kernarg_layout_matches_code_object_and_header():
    """SafeStepsTermArgs: the k_safe_steps_traj block (424 B), then term_obs
    (8 B at 424): 432 B, the header's macro."""
    from rcbf_amd import _lib
    want = [(8 * i, 8) for i in range(16)] + [(128, 4), (136, 8), (144, 8), (152, ctypes.sizeof(_lib.RcbfParams)),
                                              (392, 4), (396, 4), (400, 4), (404, 4), (408, 4), (416, 8), (424, 8)]
    defs = _header_defs()
    size = defs["RCBF_AQL_SAFE_STEPS_TERM_KERNARG_BYTES"]
    assert size == 432 == defs["RCBF_AQL_SAFE_STEPS_TRAJ_KERNARG_BYTES"] + 8
    ks = _term_kernels()
    assert ks
    for k in ks:
        assert k[".kernarg_segment_size"] == size, k[".name"]
        assert [(a[".offset"], a[".size"]) for a in k[".args"]] == want, k[".name"]
        assert all(not a[".value_kind"].startswith("hidden") for a in k[".args"]), k[".name"]


def test_term_kernels_use_no_scratch_and_do_not_spill():
    for k in _term_kernels():
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k[".vgpr_count"] <= 512, k[".name"]  # the unified file: vector and accumulation registers together
    bad = {k[".name"]: (k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in _term_kernels()
           if k[".sgpr_spill_count"] or k[".vgpr_spill_count"]}
    assert not bad, bad


def test_one_term_kernel_per_mode_and_workgroup_size():
    names = sorted(k[".name"] for k in _term_kernels())
    assert len(names) == 27
    got = {tuple(int(v) for v in re.match(TERM_PREFIX + r"Li(\d+)ELi(\d+)ELi(\d+)EEEv", n).groups()) for n in names}
    from rcbf_amd import _lib
    want = {(_lib.MODE_SIMULATED_CARS, 1, bs) for bs in (64, 128, 256)}
    want |= {(_lib.MODE_UNICYCLE, k, bs) for k in range(1, 9) for bs in (64, 128, 256)}
    assert got == want


def test_term_kernels_leave_the_other_families_prefixes_alone():
    from test_abi_fused_cpu import FUSED_PREFIX
    from test_abi_traj_cpu import TRAJ_PREFIX
    assert all(not k[".name"].startswith((FUSED_PREFIX, TRAJ_PREFIX)) for k in _term_kernels())


@pytest.fixture(scope="module")
def term_code():
    """{kernel name: [(mnemonic, operands, address), ...]} of the 27 kernels."""
    names = {k[".name"] for k in _term_kernels()}  # skips when the code object is not built
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", TERM_CO], check=True, capture_output=True,
                         text=True).stdout
    code, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), []) if m.group(1) in names else None
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = line.split("//")[0].split()
        adr = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if ins and adr:
            cur.append((ins[0], " ".join(ins[1:]), int(adr.group(1), 16)))
    assert set(code) == names and len(code) == 27
    return code


def test_no_flat_instruction_and_no_scratch_access_in_any_term_kernel(term_code):
    bad = {name: sorted({m for m, _, _ in ins if m.startswith(("flat_", "scratch_", "buffer_"))})
           for name, ins in term_code.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad
    for name, ins in term_code.items():
        ms = [m for m, _, _ in ins]
        assert len(ins) > 500 and "s_endpgm" in ms, name
        # the trajectory kernel's stores and the terminal row's (dwords, which the compiler may merge)
        assert sum(m.startswith("global_store_") for m in ms) >= 15 + 1, name
        assert any(m.startswith("global_atomic_or") for m in ms), name


def test_the_step_loop_holds_every_store_of_a_term_kernel(term_code):
    for name, ins in term_code.items():
        loop = _loop_addresses(ins)
        out = [(m, hex(a)) for m, _, a in ins if m.startswith(("global_store_", "global_atomic_")) and a not in loop]
        assert not out, (name, out)
        assert len(loop) > len(ins) // 2, name


def test_no_full_vmcnt_wait_in_the_step_loop_of_a_term_kernel(term_code):
    bad = {}
    for name, ins in term_code.items():
        loop = _loop_addresses(ins)
        full = [hex(a) for m, ops, a in ins if a in loop and m == "s_waitcnt" and re.search(r"vmcnt\(0\)", ops)]
        if full:
            bad[name] = full
        assert any(m == "s_waitcnt" and "vmcnt(0)" in ops for m, ops, a in ins if a not in loop), name
    assert not bad, bad


def test_term_obs_bit_matches_the_python_mirror_and_stays_out_of_traj_bits():
    from rcbf_amd import aql
    from rcbf_amd.envs import BatchedEnv
    assert _header_defs()["RCBF_TRAJ_TERM_OBS"] == 128 == aql.TRAJ_TERM_OBS
    assert "term_obs" not in aql.TRAJ_BITS and aql.TRAJ_TERM_OBS not in aql.TRAJ_BITS.values()
    assert "term_obs" not in BatchedEnv.TRAJECTORY_FIELDS


def _null_args(fn):
    args = [None] * len(fn.argtypes)
    for j, t in enumerate(fn.argtypes):
        if t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64):
            args[j] = 0
        elif t is ctypes.c_double:
            args[j] = 0.0
    return args


def test_term_plan_rejects_a_null_queue():
    from rcbf_amd import _lib
    lib = _lib.load()
    args = _null_args(lib.rcbf_aql_safe_step_term_plan)
    h = ctypes.c_void_p()
    args[-1] = ctypes.byref(h)
    assert lib.rcbf_aql_safe_step_term_plan(*args) == E_NULL
    assert not h.value


def test_pack_replay_rejects_bad_arguments_without_a_gpu():
    from rcbf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # 16-byte aligned host memory: never dereferenced, no launch is reached

    def call(ring=p, cap=8, pos=0, B=4, K=2, P=4, n_o=10, n_u=1, obs0=p, step0=p, obs=p, term=None, u=p, rew=p,
             done=p):
        return lib.rcbf_traj_pack_replay_f64(ring, cap, pos, B, K, P, n_o, n_u, obs0, step0, obs, term, u, rew, done,
                                             300, 0.02, 1, None)

    assert call(B=0) == 0  # an empty batch is a no-op
    assert call(B=0, ring=None) == 0
    for kw in ({"P": 3}, {"K": 0}, {"K": -1}, {"cap": 0}, {"pos": -1}, {"pos": 8}, {"B": -1}, {"n_o": 9},
               {"n_o": 7, "n_u": 1}, {"n_o": 10, "n_u": 2}):
        assert call(**kw) == E_BAD_SHAPE, kw
    for f in ("ring", "obs0", "step0", "obs", "u", "rew", "done"):
        assert call(**{f: None}) == E_NULL, f
    # cars rows are read as 8-byte pairs
    odd = ctypes.c_void_p(p.value + 4)
    for f in ("obs0", "obs", "term"):
        assert call(**{f: odd}) == E_BAD_SHAPE, f


class _StubEnv:
    """What push_trajectory reads of an env, without a device."""
    num_envs, n_o, n_u, max_episode_steps, dt = 4, 10, 1, 300, 0.02

    def _trajectory_spec(self):
        import torch
        return {"obs": (10, torch.float32), "u": (1, torch.float32), "reward": (0, torch.float32),
                "done": (0, torch.uint8), "term_obs": (10, torch.float32)}


def test_push_trajectory_checks_its_arguments_before_any_library_call(monkeypatch):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.replay_memory import ReplayMemory

    def no_library():
        raise AssertionError("push_trajectory reached the library")

    monkeypatch.setattr(_lib, "load", no_library)
    env = _StubEnv()
    mem = ReplayMemory(100, 0, device="cpu")  # host tensors stand in: every check below fails before a launch
    K, B = 3, 4

    def traj(P=64):
        return {"obs": torch.zeros(K, P, 10)[:, :B], "u": torch.zeros(K, P, 1)[:, :B],
                "reward": torch.zeros(K, P)[:, :B], "done": torch.zeros(K, P, dtype=torch.uint8)[:, :B]}

    obs0, step0 = torch.zeros(B, 10), torch.zeros(B, dtype=torch.int32)
    for f in ("obs", "u", "reward", "done"):
        t = traj()
        del t[f]
        with pytest.raises(ValueError, match=f):
            mem.push_trajectory(env, t, obs0, step0)
    t = traj()
    t["reward"] = torch.zeros(K, 128)[:, :B]  # another pitch
    with pytest.raises(ValueError, match="pitch"):
        mem.push_trajectory(env, t, obs0, step0)
    t = traj()
    t["done"] = t["done"].to(torch.int32)  # dtype
    with pytest.raises(ValueError, match="done"):
        mem.push_trajectory(env, t, obs0, step0)
    t = traj()
    t["obs"] = torch.zeros(K, B, 12)[:, :, :10]  # not dense in w
    with pytest.raises(ValueError, match="obs"):
        mem.push_trajectory(env, t, obs0, step0)
    t = traj()
    t["term_obs"] = torch.zeros(K - 1, 64, 10)[:, :B]  # fewer rows than the others are asked for
    with pytest.raises(ValueError, match="term_obs"):
        mem.push_trajectory(env, t, obs0, step0, rows=K)
    with pytest.raises(ValueError, match="rows"):
        mem.push_trajectory(env, traj(), obs0, step0, rows=K + 1)
    with pytest.raises(ValueError, match="rows"):
        mem.push_trajectory(env, traj(), obs0, step0, rows=0)
    with pytest.raises(ValueError, match="obs0"):
        mem.push_trajectory(env, traj(), obs0[:, :9], step0)
    with pytest.raises(ValueError, match="step0"):
        mem.push_trajectory(env, traj(), obs0, step0.to(torch.int64))
    assert len(mem) == 0 and mem.position == 0 and mem._ring is None
