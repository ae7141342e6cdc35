"""CPU-side checks of the cars fused plan's straight-line loop
(rcbf::k_safe_steps_fast, csrc/rcbf_safe_steps_fast.hpp) as it stands in
librcbf_steps_fast.co, the code object the AQL path dispatches it from: the
argument block is k_safe_steps's (SafeStepsArgs), nothing an AQL packet of ours
does not carry, no spill, no FLAT access; every store lies inside one of the
kernel's two loops, and each step of the first loop's iteration has all of its
own; the first loop waits for no full vmcnt and holds no library sine.  And the
reward's division by 300 through the fp64 reciprocal gives the fp32 quotient's
bits over the action box."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_abi_cpu import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
CO = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_steps_fast.co")
PREFIX = "_ZN4rcbf17k_safe_steps_fastI"


@pytest.fixture(scope="module")
def kernels():
    import yaml
    if not os.path.exists(CO):
        pytest.skip("librcbf_steps_fast.co not built")
    txt = subprocess.run([LLVM + "/llvm-readelf", "--notes", CO], check=True, capture_output=True, text=True).stdout
    m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
    assert m, "no AMDGPU metadata in librcbf_steps_fast.co"
    ks = yaml.safe_load(m.group(1))["amdhsa.kernels"]
    assert sorted(int(re.match(PREFIX + r"Li(\d+)EEEv", k[".name"]).group(1)) for k in ks) == [64, 128, 256]
    return ks


@pytest.fixture(scope="module")
def code(kernels):
    """{kernel name: [(mnemonic, operands, address), ...]}"""
    names = {k[".name"] for k in kernels}
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", CO], check=True, capture_output=True,
                         text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = line.split("//")[0].split()
        adr = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if ins and adr:
            cur.append((ins[0], " ".join(ins[1:]), int(adr.group(1), 16)))
    assert set(out) == names
    return out


def test_kernarg_block_is_safe_steps_args(kernels):
    from rcbf_amd import _lib
    want = [(8 * i, 8) for i in range(16)] + [(128, 4), (136, 8), (144, 8), (152, ctypes.sizeof(_lib.RcbfParams)),
                                              (392, 4), (396, 4), (400, 4), (404, 4)]
    for k in kernels:
        assert k[".kernarg_segment_size"] == 408, k[".name"]
        assert [(a[".offset"], a[".size"]) for a in k[".args"]] == want, k[".name"]
        assert all(not a[".value_kind"].startswith("hidden") for a in k[".args"]), k[".name"]


def test_no_scratch_and_no_spill(kernels):
    for k in kernels:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k[".sgpr_spill_count"] == 0 and k[".vgpr_spill_count"] == 0, k[".name"]


def test_no_flat_instruction(code):
    for name, ins in code.items():
        assert not sorted({m for m, _, _ in ins if m.startswith("flat_")}), name


def _loops(ins):
    """The kernel's loops as address intervals, in address order: the interval [target, branch] of every
    backward branch, overlapping intervals merged (a loop's cold blocks are laid out behind it and branch back
    into it).  A branch's target is its own address + 4 + 4 x its signed 16-bit operand."""
    back = []
    for m, ops, adr in ins:
        if m.startswith(("s_cbranch_", "s_branch")) and ops.isdigit():
            imm = int(ops)
            tgt = adr + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)
            if tgt <= adr:
                back.append([tgt, adr])
    merged = []
    for lo, hi in sorted(back):
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return merged


def _step_loops(ins):
    """(first loop, second loop): the two loops that store."""
    with_stores = [(lo, hi) for lo, hi in _loops(ins)
                   if any(m.startswith("global_store_") and lo <= a <= hi for m, _, a in ins)]
    assert len(with_stores) == 2, with_stores
    return with_stores


def test_every_store_lies_inside_a_loop(code):
    for name, ins in code.items():
        loops = _step_loops(ins)
        out = [(m, hex(a)) for m, _, a in ins if m.startswith(("global_store_", "global_atomic_"))
               and not any(lo <= a <= hi for lo, hi in loops)]
        assert not out, (name, out)
        assert sum(m.startswith("global_atomic_or") for m, _, _ in ins) == 2, name  # the fail_flag OR, once a loop


def test_each_step_of_the_first_loop_makes_all_of_its_stores(code):
    """An iteration of the first loop is two steps in one block, and the second step overwrites what the first
    stored: 14 stores a step (five state pairs, aux, step, u, reward, cost, done, three observation chunks) and
    the episode counter's in each step's reset block -- none dropped as dead."""
    for name, ins in code.items():
        lo, hi = _step_loops(ins)[0]
        st = [m for m, _, a in ins if lo <= a <= hi and m.startswith("global_store_")]
        assert len(st) == 2 * 14 + 2, (name, len(st))
        assert st.count("global_store_dwordx4") == 2 * (5 + 3), name
        assert st.count("global_store_byte") == 2, name


def test_first_loop_waits_for_no_full_vmcnt_and_has_no_library_sine(code):
    """... while the second loop, safe_step_body's, has the library sine's argument reduction: the loops are
    told apart, and a wave out of the series' range has somewhere to go."""
    for name, ins in code.items():
        (lo, hi), (lo2, hi2) = _step_loops(ins)
        first = [(m, ops) for m, ops, a in ins if lo <= a <= hi]
        assert len(first) > 1000, name
        assert not [ops for m, ops in first if m == "s_waitcnt" and "vmcnt(0)" in ops], name
        assert not [m for m, _ in first if m == "v_trig_preop_f64"], name
        assert any(m == "v_trig_preop_f64" for m, _, a in ins if lo2 <= a <= hi2), name
        assert any(m == "s_waitcnt" and "vmcnt(0)" in ops for m, ops, a in ins if a < lo), name  # the prologue's


def test_reward_division_by_reciprocal_equals_the_fp32_quotient():
    """cars_env_post<float, true>: (-5 a^2) / 300 as float(double(-5 a^2) * (1.0 / 300.0)) -- the fp32 quotient's
    bits for every safe action tried: 2^24 + 1 evenly spaced over the box [-10, 10], 2^22 random ones, and every
    fp32 in [1, 1 + 2^-4) scaled to four binades."""
    rng = np.random.default_rng(0)
    a = np.concatenate([np.linspace(-10.0, 10.0, 2 ** 24 + 1).astype(np.float32),
                        rng.uniform(-10, 10, 2 ** 22).astype(np.float32),
                        *[(np.arange(2 ** 19, dtype=np.uint32) | np.uint32(127 << 23))
                          .view(np.float32) * np.float32(s) for s in (0.01, 0.5, 1.0, 8.0)]])
    assert float(np.abs(a).max()) <= 10.0
    num = np.float32(-5.0) * np.abs(a * a)
    assert num.dtype == np.float32
    want = num / np.float32(300.0)
    got = (num.astype(np.float64) * (1.0 / 300.0)).astype(np.float32)
    assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32))


def test_flag_and_forms_match_the_python_mirror():
    from rcbf_amd import aql
    src = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RCBF_AQL_\w+)\s+(\d+)\b", src)}
    assert defs["RCBF_AQL_FUSED_LOOP"] == 256 == aql.FUSED_LOOP == 2 * defs["RCBF_AQL_PER_STEP"]
    assert [defs["RCBF_AQL_FORM_" + f.upper()] for f in aql.FORMS] == [0, 1, 2]
    assert re.search(r"#define\s+RCBF_ABI_VERSION\s+13\b", src)
    from rcbf_amd import _lib
    assert _lib.load().rcbf_aql_plan_form(None) == 1003  # RCBF_E_NULL
