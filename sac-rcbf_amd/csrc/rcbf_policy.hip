// rcbf_policy.hip -- the actor's inference forward (rcbf_sac/model.py:86-106,
// the network behind agent.select_action, sac_cbf.py:72-75) as one launch.
//
//   h1 = relu(W1 obs + b1);  h2 = relu(W2 h1 + b2)
//   mean = Wm h2 + bm;       log_std = clamp(Ws h2 + bs, -20, 2)
//   RCBF_POLICY_MEAN:    u = tanh(mean) * scale + bias
//   RCBF_POLICY_SAMPLE:  u = tanh(mean + exp(log_std) * z) * scale + bias
//
// fp32 like the reference.  Every sum is ONE fp32 fmaf chain with the bias as
// its first value and k ascending from 0 (n_o padded with a zero column to an
// even count): the two hidden layers on the fp32 MFMA (v_mfma_f32_32x32x2_f32,
// which is bit for bit that chain: exact products, one rounding per step, k0
// before k1), the heads (<= 4 outputs) on the VALU in the same order.  So a
// row's action depends on that row alone -- not on B, not on the row's place
// in the batch, not on the tile shape the launch picks.
//
// One workgroup of four waves per tile of 32 NRB rows (NRB = 1 while the batch
// leaves CUs idle, 2 beyond).  The products are formed transposed, out^T =
// W act^T: the weights are the A operand (row = output unit), the activations
// the B operand (column = batch row), so the result has the batch row on the
// lane and the units in the 16 registers, and goes to LDS as [unit][row] with
// unit-contiguous lanes -- exactly what the next layer's B operand reads
// (k = unit, 32 consecutive rows), without bank conflicts either way.  Wave w
// owns unit blocks 2w and 2w + 1 (32 units each) of a layer's output for all
// NRB row blocks.  The packed weights (rcbf_hip.h) are in the A-operand lane
// order, so a wave's weight load is one contiguous 256-B (W1) or 1-KiB (W2,
// four k-steps per lane) read from L2; W2 is never held in LDS.  Rows past B
// are computed on the last row's data and not stored: no conditional loads.
//
// Two kernel families share the body (policy_tile in rcbf_policy_tile.hpp, which rcbf_critic.hip builds on too):
// k_policy_act, which rcbf_policy_act launches through HIP, and rcbf::k_policy_step, which no HIP launch uses: csrc/rcbf_aql.hip dispatches it from librcbf_policy.co, this
// file's gfx950 code object, as the policy packets of a closed-loop plan (rcbf_aql_closed_loop_plan).
#include "rcbf_common.hpp"
#include "rcbf_policy_step.hpp"
#include "rcbf_policy_tile.hpp"

using namespace rcbf;

namespace {

struct PolicyLayout {
    int K1;  // n_o padded to even
    int64_t w1, b1, w2, b2, wm, bm, ws, bs, scale, bias, total;
};

inline PolicyLayout policy_layout(int n_o, int n_u, int H) {
    PolicyLayout L;
    L.K1 = n_o + (n_o & 1);
    L.w1 = 0;
    L.b1 = L.w1 + (int64_t)H * L.K1;
    L.w2 = L.b1 + H;
    L.b2 = L.w2 + (int64_t)H * H;
    L.wm = L.b2 + H;
    L.bm = L.wm + (int64_t)n_u * H;
    L.ws = L.bm + 4;
    L.bs = L.ws + (int64_t)n_u * H;
    L.scale = L.bs + 4;
    L.bias = L.scale + 4;
    L.total = L.bias + 4;
    return L;
}

template <bool SAMPLE, int NRB>
__global__ void __launch_bounds__(256) k_policy_act(const float* __restrict__ packed, int n_o, int n_u, int H,
                                                    int64_t B, const float* __restrict__ obs,
                                                    float* __restrict__ u_rl, const float* __restrict__ z,
                                                    uint64_t seed, uint64_t counter, int64_t env_offset) {
    policy_tile<SAMPLE, NRB>(packed, n_o, n_u, H, B, obs, u_rl, z, seed, counter, env_offset);
}

template <bool SAMPLE, int NRB>
int policy_launch(const float* packed, int n_o, int n_u, int H, int64_t B, const float* obs, float* u_rl,
                  const float* z, uint64_t seed, uint64_t counter, int64_t env_offset, hipStream_t stream) {
    const size_t lds = policy_lds_bytes(H, NRB);
    // dynamic LDS above the default 64 KiB must be opted into per kernel: once per device and size
    if (lds > 65536) {
        static std::atomic<int> allowed[64];
        int dev = 0;
        const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
        if (!known || allowed[dev].load(std::memory_order_relaxed) < (int)lds) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_policy_act<SAMPLE, NRB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
            if (known) allowed[dev].store((int)lds, std::memory_order_relaxed);
        }
    }
    const unsigned grid = (unsigned)((B + 32 * NRB - 1) / (32 * NRB));
    hipLaunchKernelGGL((k_policy_act<SAMPLE, NRB>), dim3(grid), dim3(256), lds, stream, packed, n_o, n_u, H, B, obs,
                       u_rl, z, seed, counter, env_offset);
    return launch_status();
}

}  // namespace

namespace rcbf {

// The policy packet of a closed-loop AQL plan (PolicyStepArgs, rcbf_policy_step.hpp): k_policy_act with the draw
// counter read from a device word when the packet runs -- a plan's argument blocks are written once, and every
// run must draw fresh noise -- plus the packet's own offset (its step index).  In-kernel draws only: no z.
// External linkage in namespace rcbf, like k_safe_step: rcbf_aql_open finds the kernels by their mangled names.
template <bool SAMPLE, int NRB>
__global__ void __launch_bounds__(256) k_policy_step(const float* __restrict__ packed, int n_o, int n_u, int H,
                                                     int64_t B, const float* __restrict__ obs,
                                                     float* __restrict__ u_rl, uint64_t seed,
                                                     const uint64_t* __restrict__ counter_word, uint64_t counter_add,
                                                     int64_t env_offset) {
    uint64_t counter = counter_add;
    if constexpr (SAMPLE) {
        if (counter_word) counter += *counter_word;
    }
    policy_tile<SAMPLE, NRB>(packed, n_o, n_u, H, B, obs, u_rl, nullptr, seed, counter, env_offset);
}

template __global__ void k_policy_step<false, 1>(const float*, int, int, int, int64_t, const float*, float*, uint64_t,
                                                 const uint64_t*, uint64_t, int64_t);
template __global__ void k_policy_step<false, 2>(const float*, int, int, int, int64_t, const float*, float*, uint64_t,
                                                 const uint64_t*, uint64_t, int64_t);
template __global__ void k_policy_step<true, 1>(const float*, int, int, int, int64_t, const float*, float*, uint64_t,
                                                const uint64_t*, uint64_t, int64_t);
template __global__ void k_policy_step<true, 2>(const float*, int, int, int, int64_t, const float*, float*, uint64_t,
                                                const uint64_t*, uint64_t, int64_t);

}  // namespace rcbf

extern "C" int64_t rcbf_policy_packed_floats(int32_t n_o, int32_t n_u, int32_t hidden) {
    if (!policy_shape_ok(n_o, n_u, hidden)) return -1;
    return policy_layout(n_o, n_u, hidden).total;
}

extern "C" int rcbf_policy_act(const float* packed, int32_t n_o, int32_t n_u, int32_t hidden, int64_t B,
                               const float* obs, float* u_rl, int32_t mode, const float* z, uint64_t seed,
                               uint64_t counter, int64_t env_offset, hipStream_t stream) {
    // B <= 2^31 - 1: every grid (a workgroup per 32 or 64 rows) is far inside the grid-x limit
    if (!policy_shape_ok(n_o, n_u, hidden) || B < 0 || B > INT32_MAX) return RCBF_E_BAD_SHAPE;
    if (mode != RCBF_POLICY_MEAN && mode != RCBF_POLICY_SAMPLE) return RCBF_E_BAD_MODE;
    if (env_offset < 0) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!packed || !obs || !u_rl) return RCBF_E_NULL;
    if ((reinterpret_cast<uintptr_t>(packed) & 15) || (reinterpret_cast<uintptr_t>(obs) & 3) ||
        (reinterpret_cast<uintptr_t>(u_rl) & 3) || (reinterpret_cast<uintptr_t>(z) & 3))
        return RCBF_E_BAD_SHAPE;
    // 32-row tiles while 64-row ones would leave CUs without a workgroup (half the chain per workgroup)
    const bool small = B <= 32 * num_cus();
    if (mode == RCBF_POLICY_SAMPLE) {
        if (small) return policy_launch<true, 1>(packed, n_o, n_u, hidden, B, obs, u_rl, z, seed, counter, env_offset, stream);
        return policy_launch<true, 2>(packed, n_o, n_u, hidden, B, obs, u_rl, z, seed, counter, env_offset, stream);
    }
    if (small) return policy_launch<false, 1>(packed, n_o, n_u, hidden, B, obs, u_rl, z, seed, counter, env_offset, stream);
    return policy_launch<false, 2>(packed, n_o, n_u, hidden, B, obs, u_rl, z, seed, counter, env_offset, stream);
}
