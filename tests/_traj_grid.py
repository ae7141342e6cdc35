"""The grid the trajectory packers and the episode statistics run a (B, K) plan
on, restated for the tests that need several steps per workgroup: each asserts
its own precondition on it, so a device with another CU count fails loudly
instead of silently testing one step per workgroup."""
import torch


def chunk(B, K):
    """Steps per workgroup the library picks for (B, K) on this device
    (traj_steps_per_workgroup in csrc/rcbf_model.hip)."""
    waves, want = (B + 63) // 64, 8 * torch.cuda.get_device_properties(0).multi_processor_count
    parts = min(1 if waves >= want else -(-want // waves), K, 65535)
    return -(-K // parts)
