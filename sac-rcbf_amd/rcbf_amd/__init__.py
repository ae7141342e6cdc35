"""rcbf_amd -- MI355X-native batched safe-env step of SAC-RCBF.

Hot path: SimulatedCars / Unicycle control-affine dynamics + the RCBF
safety-layer QP, as hand-written HIP kernels for gfx950 behind a C-ABI
(include/rcbf_hip.h, librcbf_hip.so) and the reference's own Python surfaces:

  rcbf_amd.diff_cbf_qp.CBFQPLayer       <- rcbf_sac/diff_cbf_qp.py
  rcbf_amd.cbf_qp.CascadeCBFLayer       <- rcbf_sac/cbf_qp.py
  rcbf_amd.dynamics.DynamicsModel (prior), DYNAMICS_MODE, MAX_STD <- rcbf_sac/dynamics.py
  rcbf_amd.envs.SimulatedCarsEnv / UnicycleEnv   <- envs/*_env.py
  rcbf_amd.envs.Batched*Env (+ safe_step / rollout: the fused kernels)
  rcbf_amd.build_env.build_env          <- build_env.py
  rcbf_amd.EpisodeStats (episode_stats) <- main.py:98-101,140-144, the loop's episode bookkeeping
  rcbf_amd.DevicePolicy (policy)        <- rcbf_sac/model.py:86-106, the actor's inference forward (one launch)
  rcbf_amd.evaluate_policy (evaluator)  <- main.py:146-177, the evaluation loop on B envs
  rcbf_amd.DeviceCritic (critic)        <- rcbf_sac/model.py:34-61, the twin critic's inference forward
  rcbf_amd.sac_cbf.td_target            <- rcbf_sac/sac_cbf.py:130-136, the SAC target (sample, safe action, twin Q)
"""
from . import _lib  # noqa: F401
from .critic import DeviceCritic  # noqa: F401
from .episode_stats import EpisodeStats  # noqa: F401
from .evaluator import evaluate_policy  # noqa: F401
from .policy import DevicePolicy  # noqa: F401

__version__ = "0.1.0"
