// rcbf_steps_traj.hip -- the trajectory form of the K-steps-per-dispatch kernels (rcbf::k_safe_steps_traj,
// rcbf_safe_step.hpp): cars, and the unicycle at 1 .. RCBF_MAX_HAZARDS hazards, at the three workgroup sizes.
// No HIP launch uses them: csrc/rcbf_aql.hip dispatches them from librcbf_steps_traj.co, this file's gfx950
// code object, which the build unbundles next to librcbf_steps.co and rcbf_aql_open loads into the same HSA
// executable.
//
// A translation unit of their own, not rcbf_env.hip: instantiated there, they changed the machine code of
// five k_safe_steps kernels of that file (cars at all three workgroup sizes, the unicycle at k = 1; other
// registers and instruction order in the prologue, one instruction fewer in the cars step loop), although
// no line of those kernels' source differs.  Here rcbf_env.hip compiles to the code object it compiled to
// before these kernels existed, byte for byte.
#include "rcbf_safe_step.hpp"

namespace rcbf {
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_SIMULATED_CARS, 1);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 1);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 2);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 3);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 4);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 5);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 6);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 7);
RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(RCBF_MODE_UNICYCLE, 8);
}  // namespace rcbf
