// rcbf_critic.hip -- the inference half of the SAC update (rcbf_sac/sac_cbf.py:130-136, under no_grad) around the
// safe action: the actor's sample WITH its log-probability (GaussianPolicy.sample, model.py:94-106), the twin
// critic's forward (QNetwork.forward, model.py:50-61) and the TD target on top of it, one launch each.
//
//   k_actor_sample   policy_tile (rcbf_policy_tile.hpp) with its LOGP epilogue: the action and the mean action
//                    are the values k_policy_act stores, bit for bit; log_pi is formed beside them.
//   k_critic_q       xu = [obs | act];  per net:  h1 = relu(W1 xu + b1);  h2 = relu(W2 h1 + b2);  q = w3 h2 + b3
//                    TD:  y = reward + (mask * gamma) * (min(q1, q2) - alpha * log_pi)
//
// The critic follows the actor's tile (top of rcbf_policy.hip): fp32, every sum ONE fmaf chain with the bias first
// and k ascending (n_o + n_u padded with a zero column to an even count, at most 18), the hidden layers on
// v_mfma_f32_32x32x2_f32 through the same mlp_hidden, the output unit on the VALU in the same order; one workgroup
// of four waves per 32 NRB rows, W2 streamed from L2, rows past B computed on the last row and not stored.  A
// row's Q-values and target therefore depend on that row alone.
//
// The two nets run ONE AFTER THE OTHER in the same LDS: xu^T is filled once (the concatenation happens there) and
// h1 / h2 are reused, so the workgroup needs (18 + 2 H + 2) ROWS floats -- 133 KiB at H = 256 with 64 rows, inside
// the CU's 160 KiB, where a buffer pair per net would not fit.  Wave 3 forms net 0's output unit while the others
// already run net 1's first layer: that layer writes h1 only, and h2 is not written again before the barrier
// inside mlp_hidden, which wave 3 reaches after its chain.
#include "rcbf_policy_step.hpp"
#include "rcbf_policy_tile.hpp"

using namespace rcbf;

namespace {

inline int critic_k1(int n_o, int n_u) { return (n_o + n_u + 1) & ~1; }
// one net: W1p H K1 | b1 H | W2p H H | b2 H | w3 H | b3 4
inline int64_t critic_net_floats(int K1, int H) { return (int64_t)H * (K1 + H + 3) + 4; }
// xu^T [18][ROWS], h1 and h2 [H][ROWS], q [2][ROWS]
inline size_t critic_lds_bytes(int H, int nrb) { return (size_t)(18 + 2 * H + 2) * 32 * nrb * sizeof(float); }

// dynamic LDS above the default 64 KiB must be opted into per kernel: once per device and size
int allow_dynamic_lds(const void* kernel, size_t lds, std::atomic<int>* allowed) {
    if (lds <= 65536) return 0;
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (!known || allowed[dev].load(std::memory_order_relaxed) < (int)lds) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        if (known) allowed[dev].store((int)lds, std::memory_order_relaxed);
    }
    return 0;
}

template <int NRB>
__global__ void __launch_bounds__(256) k_actor_sample(const float* __restrict__ packed, int n_o, int n_u, int H,
                                                      int64_t B, const float* __restrict__ obs,
                                                      float* __restrict__ u_rl, float* __restrict__ log_pi,
                                                      float* __restrict__ u_mean, const float* __restrict__ z,
                                                      uint64_t seed, uint64_t counter, int64_t env_offset) {
    policy_tile<true, NRB, true>(packed, n_o, n_u, H, B, obs, u_rl, z, seed, counter, env_offset, log_pi, u_mean);
}

template <int NRB>
int sample_launch(const float* packed, int n_o, int n_u, int H, int64_t B, const float* obs, float* u_rl,
                  float* log_pi, float* u_mean, const float* z, uint64_t seed, uint64_t counter, int64_t env_offset,
                  hipStream_t stream) {
    static std::atomic<int> allowed[64];
    const size_t lds = policy_lds_bytes(H, NRB);
    if (const int e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_actor_sample<NRB>), lds, allowed)) return e;
    const unsigned grid = (unsigned)((B + 32 * NRB - 1) / (32 * NRB));
    hipLaunchKernelGGL((k_actor_sample<NRB>), dim3(grid), dim3(256), lds, stream, packed, n_o, n_u, H, B, obs, u_rl,
                       log_pi, u_mean, z, seed, counter, env_offset);
    return launch_status();
}

template <bool TD, int NRB>
__global__ void __launch_bounds__(256) k_critic_q(const float* __restrict__ packed, int n_o, int n_u, int H,
                                                  int64_t B, const float* __restrict__ obs,
                                                  const float* __restrict__ act, const float* __restrict__ reward,
                                                  const float* __restrict__ mask, const float* __restrict__ log_pi,
                                                  float alpha, const float* __restrict__ alpha_dev, float gamma,
                                                  float* __restrict__ y, float* __restrict__ q1,
                                                  float* __restrict__ q2) {
    constexpr int ROWS = 32 * NRB;
    extern __shared__ __align__(16) float crt_smem[];
    float* const s_x = crt_smem;             // [18][ROWS]   [obs | act]^T, zero column when n_o + n_u is odd
    float* const s_h1 = s_x + 18 * ROWS;     // [H][ROWS]
    float* const s_h2 = s_h1 + H * ROWS;     // [H][ROWS]
    float* const s_q = s_h2 + H * ROWS;      // [2][ROWS]    q1, q2

    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int n_in = n_o + n_u, K1 = (n_in + 1) & ~1, S1 = K1 >> 1;
    const int net_floats = H * (K1 + H + 3) + 4;

    // the tile's inputs, transposed: torch.cat([state, action], 1) happens here
    for (int e = t; e < ROWS * n_in; e += 256) {
        const int r = e / n_in, k = e - r * n_in;
        const int64_t gr = row0 + r < B ? row0 + r : B - 1;
        s_x[k * ROWS + r] = k < n_o ? obs[gr * n_o + k] : act[gr * n_u + (k - n_o)];
    }
    if ((n_in & 1) && t < ROWS) s_x[n_in * ROWS + t] = 0.0f;
    __syncthreads();

#pragma unroll 1
    for (int net = 0; net < 2; ++net) {
        const float* const pw1 = packed + net * net_floats;
        const float* const pb1 = pw1 + H * K1;
        const float* const pw2 = pb1 + H;
        const float* const pb2 = pw2 + H * H;
        const float* const pw3 = pb2 + H;
        const float* const pb3 = pw3 + H;
        mlp_hidden<NRB>(s_x, s_h1, s_h2, pw1, pb1, pw2, pb2, S1, H);
        // the output unit, a row per lane, on the wave with the least MFMA work
        if (w == 3 && lane < ROWS) s_q[net * ROWS + lane] = head_chain<ROWS>(pw3, pb3[0], s_h2, H, lane);
    }
    __syncthreads();

    if (t < ROWS && row0 + t < B) {
#pragma clang fp contract(off)
        const int64_t gr = row0 + t;
        const float a = s_q[t], b = s_q[ROWS + t];
        if (q1) q1[gr] = a;
        if (q2) q2[gr] = b;
        if constexpr (TD) {
            const float mn = (b < a || b != b) ? b : a;  // torch.min: a NaN in either is kept
            const float al = alpha_dev ? *alpha_dev : alpha;
            y[gr] = reward[gr] + (mask[gr] * gamma) * (mn - al * log_pi[gr]);
        }
    }
}

template <bool TD, int NRB>
int critic_launch(const float* packed, int n_o, int n_u, int H, int64_t B, const float* obs, const float* act,
                  const float* reward, const float* mask, const float* log_pi, float alpha, const float* alpha_dev,
                  float gamma, float* y, float* q1, float* q2, hipStream_t stream) {
    static std::atomic<int> allowed[64];
    const size_t lds = critic_lds_bytes(H, NRB);
    if (const int e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_critic_q<TD, NRB>), lds, allowed)) return e;
    const unsigned grid = (unsigned)((B + 32 * NRB - 1) / (32 * NRB));
    hipLaunchKernelGGL((k_critic_q<TD, NRB>), dim3(grid), dim3(256), lds, stream, packed, n_o, n_u, H, B, obs, act,
                       reward, mask, log_pi, alpha, alpha_dev, gamma, y, q1, q2);
    return launch_status();
}

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// what rcbf_critic_q and rcbf_critic_td_target check alike; > 0: the code to return, 0: launch, -1: empty batch
int critic_check(const float* packed, int n_o, int n_u, int H, int64_t B, const float* obs, const float* act) {
    if (!policy_shape_ok(n_o, n_u, H) || B < 0 || B > INT32_MAX) return RCBF_E_BAD_SHAPE;
    if (B == 0) return -1;
    if (!packed || !obs || !act) return RCBF_E_NULL;
    if ((reinterpret_cast<uintptr_t>(packed) & 15) || misaligned4(obs) || misaligned4(act)) return RCBF_E_BAD_SHAPE;
    return 0;
}

}  // namespace

extern "C" int rcbf_policy_sample(const float* packed, int32_t n_o, int32_t n_u, int32_t hidden, int64_t B,
                                  const float* obs, float* u_rl, float* log_pi, float* u_mean, const float* z,
                                  uint64_t seed, uint64_t counter, int64_t env_offset, int32_t has_log_std,
                                  hipStream_t stream) {
    if (!policy_shape_ok(n_o, n_u, hidden) || B < 0 || B > INT32_MAX || env_offset < 0) return RCBF_E_BAD_SHAPE;
    if (!has_log_std) return RCBF_E_BAD_MODE;
    if (B == 0) return 0;
    if (!packed || !obs || !u_rl) return RCBF_E_NULL;
    if ((reinterpret_cast<uintptr_t>(packed) & 15) || misaligned4(obs) || misaligned4(u_rl) || misaligned4(log_pi) ||
        misaligned4(u_mean) || misaligned4(z))
        return RCBF_E_BAD_SHAPE;
    // rcbf_policy_act's rule: 32-row tiles while 64-row ones would leave CUs without a workgroup
    if (B <= 32 * num_cus())
        return sample_launch<1>(packed, n_o, n_u, hidden, B, obs, u_rl, log_pi, u_mean, z, seed, counter, env_offset,
                                stream);
    return sample_launch<2>(packed, n_o, n_u, hidden, B, obs, u_rl, log_pi, u_mean, z, seed, counter, env_offset,
                            stream);
}

extern "C" int64_t rcbf_critic_packed_floats(int32_t n_o, int32_t n_u, int32_t hidden) {
    if (!policy_shape_ok(n_o, n_u, hidden)) return -1;
    return 2 * critic_net_floats(critic_k1(n_o, n_u), hidden);
}

extern "C" int rcbf_critic_q(const float* packed, int32_t n_o, int32_t n_u, int32_t hidden, int64_t B,
                             const float* obs, const float* act, float* q1, float* q2, hipStream_t stream) {
    if (const int rc = critic_check(packed, n_o, n_u, hidden, B, obs, act)) return rc < 0 ? 0 : rc;
    if (!q1 || !q2) return RCBF_E_NULL;
    if (misaligned4(q1) || misaligned4(q2)) return RCBF_E_BAD_SHAPE;
    if (B <= 32 * num_cus())
        return critic_launch<false, 1>(packed, n_o, n_u, hidden, B, obs, act, nullptr, nullptr, nullptr, 0.0f,
                                       nullptr, 0.0f, nullptr, q1, q2, stream);
    return critic_launch<false, 2>(packed, n_o, n_u, hidden, B, obs, act, nullptr, nullptr, nullptr, 0.0f, nullptr,
                                   0.0f, nullptr, q1, q2, stream);
}

extern "C" int rcbf_critic_td_target(const float* packed, int32_t n_o, int32_t n_u, int32_t hidden, int64_t B,
                                     const float* obs, const float* act, const float* reward, const float* mask,
                                     const float* log_pi, float alpha, const float* alpha_dev, float gamma, float* y,
                                     float* q1, float* q2, hipStream_t stream) {
    if (const int rc = critic_check(packed, n_o, n_u, hidden, B, obs, act)) return rc < 0 ? 0 : rc;
    if (!reward || !mask || !log_pi || !y) return RCBF_E_NULL;
    if (misaligned4(reward) || misaligned4(mask) || misaligned4(log_pi) || misaligned4(alpha_dev) || misaligned4(y) ||
        misaligned4(q1) || misaligned4(q2))
        return RCBF_E_BAD_SHAPE;
    if (B <= 32 * num_cus())
        return critic_launch<true, 1>(packed, n_o, n_u, hidden, B, obs, act, reward, mask, log_pi, alpha, alpha_dev,
                                      gamma, y, q1, q2, stream);
    return critic_launch<true, 2>(packed, n_o, n_u, hidden, B, obs, act, reward, mask, log_pi, alpha, alpha_dev,
                                  gamma, y, q1, q2, stream);
}
