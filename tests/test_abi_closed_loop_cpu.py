"""CPU-side checks of the closed-loop plans' policy kernels
(rcbf::k_policy_step, csrc/rcbf_policy.hip) as they stand in
librcbf_policy.co, the fourth code object rcbf_aql_open loads: the argument
block csrc/rcbf_aql.hip writes (PolicyStepArgs, csrc/rcbf_policy_step.hpp), no
hidden arguments, no scratch, no spill, no static LDS (the packet carries the
whole group segment), 256 threads; and the new entry point's symbol and its
null-queue answer, none of which needs a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from test_abi_cpu import ROOT
from test_abi_term_cpu import E_NULL, _null_args
from test_abi_traj_cpu import _header_defs

STEP_PREFIX = "_ZN4rcbf13k_policy_stepI"
POLICY_CO = os.path.join(ROOT, "sac-rcbf_amd", "rcbf_amd", "librcbf_policy.co")
# PolicyStepArgs: packed, n_o, n_u, H, (pad), B, obs, u_rl, seed, counter_word, counter_add, env_offset
ARGS = [(0, 8), (8, 4), (12, 4), (16, 4), (24, 8), (32, 8), (40, 8), (48, 8), (56, 8), (64, 8), (72, 8)]


def _step_kernels():
    import yaml
    if not os.path.exists(POLICY_CO):
        pytest.skip("librcbf_policy.co not built")
    txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", POLICY_CO], check=True,
                         capture_output=True, text=True).stdout
    m = re.search(r"^\s*---\n(.*?)^\.\.\.", txt, re.S | re.M)
    assert m, "no AMDGPU metadata in librcbf_policy.co"
    return [k for k in yaml.safe_load(m.group(1))["amdhsa.kernels"] if k[".name"].startswith(STEP_PREFIX)]


def test_four_policy_step_kernels_with_external_names():
    names = sorted(k[".name"] for k in _step_kernels())
    assert len(names) == 4, names
    got = {tuple(int(v) for v in re.match(STEP_PREFIX + r"Lb(\d)ELi(\d)EEEv", n).groups()) for n in names}
    assert got == {(s, nrb) for s in (0, 1) for nrb in (1, 2)}  # {mean, sample} x {32-row, 64-row tiles}
    assert all("k_policy_act" not in n for n in names)


def test_policy_step_kernarg_layout_matches_code_object_and_header():
    size = _header_defs()["RCBF_AQL_POLICY_STEP_KERNARG_BYTES"]
    assert size == 80
    ks = _step_kernels()
    assert len(ks) == 4
    for k in ks:
        assert k[".kernarg_segment_size"] == size, k[".name"]
        assert [(a[".offset"], a[".size"]) for a in k[".args"]] == ARGS, k[".name"]
        assert all(not a[".value_kind"].startswith("hidden") for a in k[".args"]), k[".name"]


def test_policy_step_kernels_use_no_scratch_no_static_lds_and_do_not_spill():
    ks = _step_kernels()
    assert len(ks) == 4
    for k in ks:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
        assert k[".sgpr_spill_count"] == 0 and k[".vgpr_spill_count"] == 0, k[".name"]
        assert k[".group_segment_fixed_size"] == 0, k[".name"]
        assert k[".max_flat_workgroup_size"] == 256, k[".name"]
        assert k[".vgpr_count"] <= 512, k[".name"]


def test_library_exports_the_entry_point_and_keeps_the_abi_version():
    from rcbf_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rcbf_aql_closed_loop_plan")
    assert "rcbf_aql_closed_loop_plan" in _lib.SIGNATURES
    assert lib.rcbf_abi_version() == 13 == _header_defs()["RCBF_ABI_VERSION"]


def test_closed_loop_plan_rejects_a_null_queue():
    from rcbf_amd import _lib
    lib = _lib.load()
    args = _null_args(lib.rcbf_aql_closed_loop_plan)
    h = ctypes.c_void_p()
    args[-1] = ctypes.byref(h)
    assert lib.rcbf_aql_closed_loop_plan(*args) == E_NULL
    assert not h.value


def test_python_surface_without_a_device():
    """The method and the evaluator's new arguments exist; chunk without a queue is refused before anything
    touches a device."""
    import inspect

    from rcbf_amd import aql
    from rcbf_amd.evaluator import evaluate_policy
    sig = inspect.signature(aql.AqlQueue.closed_loop_plan)
    assert list(sig.parameters)[1:] == ["env", "policy", "layer", "steps", "evaluate", "mean", "sigma", "outputs",
                                        "auto_reset", "prior_layout", "trajectory", "fence_flags"]
    assert sig.parameters["evaluate"].default is False and sig.parameters["auto_reset"].default is True
    assert issubclass(aql.ClosedLoopPlan, aql.AqlPlan)
    ev = inspect.signature(evaluate_policy).parameters
    assert ev["queue"].default is None and ev["chunk"].default is None
