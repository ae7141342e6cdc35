// rcbf_steps_fast.hip -- the cars fused plan's straight-line loop (rcbf::k_safe_steps_fast,
// rcbf_safe_steps_fast.hpp) at the three workgroup sizes.  No HIP launch uses these kernels: csrc/rcbf_aql.hip
// dispatches them from librcbf_steps_fast.co, this file's gfx950 code object, which the build unbundles next to
// librcbf_steps.co and rcbf_aql_open loads into an HSA executable of its own.
//
// A translation unit of their own for the reason rcbf_steps_traj.hip gives: the other code objects compile to
// the bytes they compiled to before these kernels existed.
#include "rcbf_safe_steps_fast.hpp"

namespace rcbf {
RCBF_SAFE_STEPS_FAST_INSTANTIATE(64);
RCBF_SAFE_STEPS_FAST_INSTANTIATE(128);
RCBF_SAFE_STEPS_FAST_INSTANTIATE(256);
}  // namespace rcbf
