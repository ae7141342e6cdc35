// rcbf_policy_step.hpp -- what rcbf_policy.hip (the kernels) and rcbf_aql.hip (the packets of a closed-loop plan)
// share: the shapes the policy kernels take, the dynamic LDS a tile needs, and the argument block of
// rcbf::k_policy_step.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rcbf_hip.h"

namespace rcbf {

inline bool policy_shape_ok(int n_o, int n_u, int H) {
    return n_o >= 1 && n_o <= 16 && n_u >= 1 && n_u <= 2 && H >= 32 && H <= 256 && H % 32 == 0;
}

// dynamic LDS of one workgroup: obs^T [16][ROWS], h1 and h2 [H][ROWS], the head outputs [4][ROWS], ROWS = 32 nrb
inline size_t policy_lds_bytes(int H, int nrb) { return (size_t)(16 + 2 * H + 4) * 32 * nrb * sizeof(float); }

// Kernel-argument block of rcbf::k_policy_step<SAMPLE, NRB> (rcbf_policy.hip), in the order and at the offsets of
// its parameter list (every argument at its natural alignment).  The kernel reads no hidden arguments:
// rcbf_aql_open checks the size against the loaded code object, tests/test_abi_closed_loop_cpu.py the offsets
// against the metadata of librcbf_policy.co.
struct PolicyStepArgs {
    const float* packed;
    int32_t n_o;
    int32_t n_u;
    int32_t H;
    int64_t B;
    const float* obs;
    float* u_rl;
    uint64_t seed;
    const uint64_t* counter_word;  // nullable: the draw counter is *counter_word + counter_add, else counter_add
    uint64_t counter_add;
    int64_t env_offset;
};
static_assert(offsetof(PolicyStepArgs, packed) == 0 && offsetof(PolicyStepArgs, n_o) == 8 &&
                  offsetof(PolicyStepArgs, n_u) == 12 && offsetof(PolicyStepArgs, H) == 16,
              "kernarg layout");
static_assert(offsetof(PolicyStepArgs, B) == 24 && offsetof(PolicyStepArgs, obs) == 32 &&
                  offsetof(PolicyStepArgs, u_rl) == 40 && offsetof(PolicyStepArgs, seed) == 48,
              "kernarg layout");
static_assert(offsetof(PolicyStepArgs, counter_word) == 56 && offsetof(PolicyStepArgs, counter_add) == 64 &&
                  offsetof(PolicyStepArgs, env_offset) == 72,
              "kernarg layout");
static_assert(sizeof(PolicyStepArgs) == RCBF_AQL_POLICY_STEP_KERNARG_BYTES, "kernarg layout");

}  // namespace rcbf
