// rcbf_steps_term.hip -- the trajectory kernels that also keep the TERMINAL observation (rcbf::k_safe_steps_term,
// rcbf_safe_step.hpp; RCBF_TRAJ_TERM_OBS): cars, and the unicycle at 1 .. RCBF_MAX_HAZARDS hazards, at the three
// workgroup sizes.  No HIP launch uses them: csrc/rcbf_aql.hip dispatches them from librcbf_steps_term.co, this
// file's gfx950 code object, which the build unbundles next to librcbf_steps.co and librcbf_steps_traj.co and
// rcbf_aql_open loads into an HSA executable of its own.
//
// A translation unit of their own for the reason rcbf_steps_traj.hip gives: rcbf_env.hip and rcbf_steps_traj.hip
// compile to the code objects they compiled to before these kernels existed, byte for byte.
#include "rcbf_safe_step.hpp"

namespace rcbf {
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_SIMULATED_CARS, 1);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 1);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 2);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 3);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 4);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 5);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 6);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 7);
RCBF_SAFE_STEPS_TERM_INSTANTIATE(RCBF_MODE_UNICYCLE, 8);
}  // namespace rcbf
