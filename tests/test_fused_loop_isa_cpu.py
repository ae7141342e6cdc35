"""The machine code of the fused plan form's kernels (rcbf::k_safe_steps in
csrc/rcbf_safe_step.hpp) as it stands in librcbf_steps.co, disassembled with
the llvm-objdump of the ROCm the build uses.

Every memory access of these kernels is a global_* (or scalar, or LDS)
instruction: a FLAT access counts in vmcnt and lgkmcnt at once and can only be
waited for with a full (0).  And the step loop, found as the largest region
closed by backward branches, holds no `s_waitcnt vmcnt(0)`: vmcnt counts loads
and stores in order, so in a loop that never ends its kernel such a wait, for
whatever load, also waits for every store of the step before."""
import os
import re
import subprocess

import pytest

from test_abi_cpu import ROOT
from test_abi_fused_cpu import FUSED_PREFIX, _fused_kernels

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def fused_code():
    """{kernel name: [(mnemonic, operands, address), ...]} of the 27 k_safe_steps kernels."""
    names = {k[".name"] for k in _fused_kernels()}  # skips when the code object is not built
    co = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_steps.co")
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
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
    assert set(code) == names
    return code


def test_all_27_fused_kernels_are_disassembled(fused_code):
    assert len(fused_code) == 27
    assert all(n.startswith(FUSED_PREFIX) for n in fused_code)
    for name, ins in fused_code.items():
        assert len(ins) > 500 and any(m == "s_endpgm" for m, _, _ in ins), name


def test_no_flat_instruction_in_any_fused_kernel(fused_code):
    bad = {name: sorted({m for m, _, _ in ins if m.startswith("flat_")}) for name, ins in fused_code.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, bad


def test_every_fused_kernel_stores_and_loads_through_global_instructions(fused_code):
    """The same kernels do have the stores and the action load (the check
    above is not passing on an empty or mis-parsed listing)."""
    for name, ins in fused_code.items():
        ms = [m for m, _, _ in ins]
        assert sum(m.startswith("global_store_") for m in ms) >= 15, name
        assert any(m.startswith("global_load_") for m in ms), name
        assert any(m.startswith("global_atomic_or") for m in ms), name  # the fail_flag OR


def _step_loop(ins):
    """(first, last) address of the step loop: the widest interval [target,
    branch] of a backward branch, grown by every backward branch interval that
    overlaps it (a rotated loop has its latch block ahead of its header, and
    several blocks branch back).  A branch's target is its own address + 4 +
    4 x its signed 16-bit operand."""
    back = []
    for m, ops, adr in ins:
        if m.startswith(("s_cbranch_", "s_branch")) and ops.isdigit():
            imm = int(ops)
            tgt = adr + 4 + 4 * (imm - 65536 if imm >= 32768 else imm)
            if tgt <= adr:
                back.append((tgt, adr))
    assert back, "no backward branch"
    lo, hi = max(back, key=lambda iv: iv[1] - iv[0])
    grown = True
    while grown:
        grown = False
        for t, a in back:
            if t <= hi and a >= lo and (t < lo or a > hi):
                lo, hi, grown = min(lo, t), max(hi, a), True
    return lo, hi


def test_the_step_loop_holds_every_store(fused_code):
    """The region the next test scans is the step loop: every store and the
    fail_flag OR of a fused kernel lie inside it, and it is most of the kernel."""
    for name, ins in fused_code.items():
        lo, hi = _step_loop(ins)
        out = [(m, hex(a)) for m, _, a in ins if m.startswith(("global_store_", "global_atomic_")) and not lo <= a <= hi]
        assert not out, (name, out)
        assert sum(lo <= a <= hi for _, _, a in ins) > len(ins) // 2, name


def test_no_full_vmcnt_wait_anywhere_in_the_step_loop(fused_code):
    """From the loop's first instruction (its header, or the latch block laid
    out ahead of it) to its last backward branch no `s_waitcnt vmcnt(0)`, in
    all 27 kernels: the next step's action is waited for with a counted
    vmcnt(N) that leaves this step's stores in flight, the table entry comes
    through a scalar load, the episode counter is not re-read, and at k = 8 the
    parameter block is read from LDS.  The prologue's own full wait stands
    ahead of the loop."""
    bad = {}
    for name, ins in fused_code.items():
        lo, hi = _step_loop(ins)
        full = [hex(a) for m, ops, a in ins if lo <= a <= hi and m == "s_waitcnt" and re.search(r"vmcnt\(0\)", ops)]
        if full:
            bad[name] = full
        assert any(m == "s_waitcnt" and "vmcnt(0)" in ops for m, ops, a in ins if a < lo), name
    assert not bad, bad
