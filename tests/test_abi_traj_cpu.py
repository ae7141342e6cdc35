"""CPU-side checks of the trajectory plan form's kernels (rcbf::k_safe_steps_traj
in csrc/rcbf_safe_step.hpp, instantiated in csrc/rcbf_steps_traj.hip) as they
stand in librcbf_steps_traj.co, the code object rcbf_aql_open loads beside
librcbf_steps.co: the argument block csrc/rcbf_aql.hip writes
(SafeStepsTrajArgs = SafeStepsArgs + traj_mask + traj_pitch), nothing an AQL
packet of ours does not carry (hidden arguments, scratch), no register spill,
one kernel per mode / hazard count and workgroup size; their machine code (no
FLAT access, every store in the step loop, no full vmcnt wait in it); the mask
bits' Python mirror and the new entry point's argument check."""
import ctypes
import os
import re
import subprocess

import pytest

from test_abi_cpu import ROOT
from test_fused_loop_isa_cpu import OBJDUMP, _step_loop

TRAJ_PREFIX = "_ZN4rcbf17k_safe_steps_trajI"
TRAJ_CO = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_steps_traj.co")


def _traj_kernels():
    """AMDGPU metadata of the k_safe_steps_traj kernels (as
    test_abi_cpu._steps_code_object_kernels reads librcbf_steps.co)."""
    import yaml
    if not os.path.exists(TRAJ_CO):
        pytest.skip("librcbf_steps_traj.co not built")
    txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", TRAJ_CO], check=True, capture_output=True,
                         text=True).stdout
    m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
    assert m, "no AMDGPU metadata in librcbf_steps_traj.co"
    return [k for k in yaml.safe_load(m.group(1))["amdhsa.kernels"] if k[".name"].startswith(TRAJ_PREFIX)]


def _header_defs():
    src = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(RCBF_\w+)\s+(\d+)\b", src)}


def test_traj_kernarg_layout_matches_code_object_and_header():
    """SafeStepsTrajArgs: the k_safe_steps block (408 B), then traj_mask (4 B
    at 408) and traj_pitch (8 B at 416): 424 B, the header's macro."""
    from rcbf_amd import _lib
    want = [(8 * i, 8) for i in range(16)] + [(128, 4), (136, 8), (144, 8), (152, ctypes.sizeof(_lib.RcbfParams)),
                                              (392, 4), (396, 4), (400, 4), (404, 4), (408, 4), (416, 8)]
    size = _header_defs()["RCBF_AQL_SAFE_STEPS_TRAJ_KERNARG_BYTES"]
    assert size == 424
    ks = _traj_kernels()
    assert ks
    for k in ks:
        assert k[".kernarg_segment_size"] == size, k[".name"]
        assert [(a[".offset"], a[".size"]) for a in k[".args"]] == want, k[".name"]
        assert all(not a[".value_kind"].startswith("hidden") for a in k[".args"]), k[".name"]


def test_traj_kernels_use_no_scratch_and_do_not_spill():
    for k in _traj_kernels():
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
    bad = {k[".name"]: (k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in _traj_kernels()
           if k[".sgpr_spill_count"] or k[".vgpr_spill_count"]}
    assert not bad, bad


def test_one_traj_kernel_per_mode_and_workgroup_size():
    names = sorted(k[".name"] for k in _traj_kernels())
    assert len(names) == 27
    got = {tuple(int(v) for v in re.match(TRAJ_PREFIX + r"Li(\d+)ELi(\d+)ELi(\d+)EEEv", n).groups()) for n in names}
    from rcbf_amd import _lib
    want = {(_lib.MODE_SIMULATED_CARS, 1, bs) for bs in (64, 128, 256)}
    want |= {(_lib.MODE_UNICYCLE, k, bs) for k in range(1, 9) for bs in (64, 128, 256)}
    assert got == want


def test_traj_kernels_leave_the_fused_kernels_prefix_alone():
    """The new family has its own name: nothing in the new code object starts
    with the k_safe_steps prefix the existing tests count."""
    from test_abi_fused_cpu import FUSED_PREFIX
    assert all(not k[".name"].startswith(FUSED_PREFIX) for k in _traj_kernels())


@pytest.fixture(scope="module")
def traj_code():
    """{kernel name: [(mnemonic, operands, address), ...]} of the 27 kernels."""
    names = {k[".name"] for k in _traj_kernels()}  # skips when the code object is not built
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", TRAJ_CO], check=True, capture_output=True,
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


def test_no_flat_instruction_and_no_scratch_access_in_any_traj_kernel(traj_code):
    bad = {name: sorted({m for m, _, _ in ins if m.startswith(("flat_", "scratch_", "buffer_"))})
           for name, ins in traj_code.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad
    for name, ins in traj_code.items():  # ... and the listing is not empty or mis-parsed
        ms = [m for m, _, _ in ins]
        assert len(ins) > 500 and "s_endpgm" in ms, name
        assert sum(m.startswith("global_store_") for m in ms) >= 15, name
        assert any(m.startswith("global_load_") for m in ms), name
        assert any(m.startswith("global_atomic_or") for m in ms), name


def _loop_addresses(ins):
    """Addresses of the step loop's instructions: the largest strongly
    connected component of the kernel's control-flow graph.  _step_loop (the
    widest backward-branch interval, grown by overlapping ones) bounds it from
    outside, which is asserted, but is not tight here: these kernels keep
    blocks of their PROLOGUE (the optional prior loads) behind the loop, each
    returning with a backward branch into the prologue that closes no cycle."""
    addr = [a for _, _, a in ins]
    index = {a: j for j, a in enumerate(addr)}
    succ = [[] for _ in ins]
    for j, (m, ops, a) in enumerate(ins):
        branch = m.startswith(("s_cbranch_", "s_branch"))
        assert not m.startswith(("s_setpc", "s_swappc", "s_call")), (m, hex(a))
        if branch:
            assert ops.isdigit(), (m, ops)
            imm = int(ops)
            succ[j].append(index[a + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)])
        if m not in ("s_branch", "s_endpgm") and j + 1 < len(ins):
            succ[j].append(j + 1)
    # Tarjan, iteratively
    n = len(ins)
    num, low, on, stack, comps, cnt = [-1] * n, [0] * n, [False] * n, [], [], 0
    for root in range(n):
        if num[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                num[v] = low[v] = cnt
                cnt += 1
                stack.append(v)
                on[v] = True
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if num[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], num[w])
                continue
            if low[v] == num[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                comps.append(comp)
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    loop = {addr[j] for j in max(comps, key=len)}
    lo, hi = _step_loop(ins)
    assert all(lo <= a <= hi for a in loop)
    return loop


def test_the_step_loop_holds_every_store_of_a_traj_kernel(traj_code):
    for name, ins in traj_code.items():
        loop = _loop_addresses(ins)
        out = [(m, hex(a)) for m, _, a in ins if m.startswith(("global_store_", "global_atomic_")) and a not in loop]
        assert not out, (name, out)
        assert len(loop) > len(ins) // 2, name


def test_no_full_vmcnt_wait_in_the_step_loop_of_a_traj_kernel(traj_code):
    """Advancing the recorded pointers at a step's end waits for nothing: the
    mask and the pitch come through scalar loads (LDS at k = 8).  The
    prologue's own full wait stands outside the loop."""
    bad = {}
    for name, ins in traj_code.items():
        loop = _loop_addresses(ins)
        full = [hex(a) for m, ops, a in ins if a in loop and m == "s_waitcnt" and re.search(r"vmcnt\(0\)", ops)]
        if full:
            bad[name] = full
        assert any(m == "s_waitcnt" and "vmcnt(0)" in ops for m, ops, a in ins if a not in loop), name
    assert not bad, bad


def test_traj_mask_bits_match_the_python_mirror():
    from rcbf_amd import aql
    defs = _header_defs()
    want = {"obs": 1, "u": 2, "reward": 4, "cost": 8, "done": 16, "goal_met": 32, "status": 64}
    assert {f: defs["RCBF_TRAJ_" + f.upper()] for f in want} == want == aql.TRAJ_BITS
    assert (aql.TRAJ_OBS, aql.TRAJ_U, aql.TRAJ_REWARD, aql.TRAJ_COST, aql.TRAJ_DONE, aql.TRAJ_GOAL_MET,
            aql.TRAJ_STATUS) == (1, 2, 4, 8, 16, 32, 64)


def test_traj_plan_rejects_a_null_queue():
    from rcbf_amd import _lib
    lib = _lib.load()
    n = len(lib.rcbf_aql_safe_step_traj_plan.argtypes)
    args = [None] * n
    for j, t in enumerate(lib.rcbf_aql_safe_step_traj_plan.argtypes):
        if t in (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64):
            args[j] = 0
    h = ctypes.c_void_p()
    args[-1] = ctypes.byref(h)
    assert lib.rcbf_aql_safe_step_traj_plan(*args) == 1003  # RCBF_E_NULL
    assert not h.value
