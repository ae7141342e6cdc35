"""CPU-side checks of the fused plan form's kernels (rcbf::k_safe_steps in
csrc/rcbf_safe_step.hpp) as they stand in librcbf_steps.co, the code object
the AQL path dispatches from: the argument block csrc/rcbf_aql.hip writes
(SafeStepsArgs), nothing an AQL packet of ours does not carry (hidden
arguments, scratch), no register spill, one kernel per mode / hazard count
and workgroup size; plus the new flag's Python mirror and the new entry
point's argument check."""
import ctypes
import os
import re

import pytest

from test_abi_cpu import ROOT, _steps_code_object_kernels

FUSED_PREFIX = "_ZN4rcbf12k_safe_stepsI"


def _fused_kernels():
    return [k for k in _steps_code_object_kernels() if k[".name"].startswith(FUSED_PREFIX)]


def test_fused_kernarg_layout_matches_code_object():
    """SafeStepsArgs: k_safe_step's block with the u_RL pointer table in
    u_rl's place and n_u, steps, ju0 (4 B each) where the stamp pointer was."""
    from rcbf_amd import _lib
    want = [(8 * i, 8) for i in range(16)] + [(128, 4), (136, 8), (144, 8), (152, ctypes.sizeof(_lib.RcbfParams)),
                                              (392, 4), (396, 4), (400, 4), (404, 4)]
    ks = _fused_kernels()
    assert ks
    for k in ks:
        assert k[".kernarg_segment_size"] == 408, k[".name"]
        assert [(a[".offset"], a[".size"]) for a in k[".args"]] == want, k[".name"]
        assert all(not a[".value_kind"].startswith("hidden") for a in k[".args"]), k[".name"]


def test_fused_kernels_use_no_scratch():
    for k in _fused_kernels():
        assert k[".private_segment_fixed_size"] == 0, k[".name"]


def test_fused_kernels_do_not_spill():
    """No scalar or vector register spill in any of the 27 kernels, the
    unicycle at 7 and 8 hazards included, whose single step already takes
    every scalar and vector register (the loop's own values live in
    accumulation registers for that, see k_safe_steps)."""
    bad = {k[".name"]: (k[".sgpr_spill_count"], k[".vgpr_spill_count"]) for k in _fused_kernels()
           if k[".sgpr_spill_count"] or k[".vgpr_spill_count"]}
    assert not bad, bad


def test_one_fused_kernel_per_mode_and_workgroup_size():
    names = sorted(k[".name"] for k in _fused_kernels())
    assert len(names) == 27
    got = {tuple(int(v) for v in re.match(FUSED_PREFIX + r"Li(\d+)ELi(\d+)ELi(\d+)EEEv", n).groups()) for n in names}
    from rcbf_amd import _lib
    want = {(_lib.MODE_SIMULATED_CARS, 1, bs) for bs in (64, 128, 256)}
    want |= {(_lib.MODE_UNICYCLE, k, bs) for k in range(1, 9) for bs in (64, 128, 256)}
    assert got == want


def test_per_step_flag_matches_the_python_mirror():
    from rcbf_amd import aql
    src = open(os.path.join(ROOT, "include", "rcbf_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RCBF_AQL_\w+)\s+(\d+)\b", src)}
    assert defs["RCBF_AQL_PER_STEP"] == 128 == aql.PER_STEP
    assert defs["RCBF_AQL_PROFILE_ENDS"] == aql.PROFILE_ENDS and defs["RCBF_AQL_PROFILE"] == aql.PROFILE
    assert defs["RCBF_AQL_SAFE_STEPS_KERNARG_BYTES"] == 408


def test_plan_dispatches_rejects_null():
    from rcbf_amd import _lib
    assert _lib.load().rcbf_aql_plan_dispatches(None) == 1003  # RCBF_E_NULL
