// rcbf_policy_tile.hpp -- the fp32-MFMA MLP tile that rcbf_policy.hip (the actor) and rcbf_critic.hip (the actor's
// sample with its log-probability, the twin critic) share: the two hidden layers of one workgroup's 32 NRB rows
// (mlp_hidden) and the actor's whole forward on top of them (policy_tile).  Layout, summation order and the
// wave-to-unit-block map are described at the top of rcbf_policy.hip.
#pragma once

#include "rcbf_common.hpp"

namespace rcbf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the accumulator of unit block cb starts as the bias: register r of lane half h holds unit
// 32 cb + (r & 3) + 8 (r >> 2) + 4 h (the C/D row map), i.e. four float4 of the bias vector
__device__ __forceinline__ f32x16 bias_acc(const float* __restrict__ b, int cb, int half) {
    f32x16 a;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(b + 32 * cb + 8 * g + 4 * half);
        a[4 * g + 0] = v.x;
        a[4 * g + 1] = v.y;
        a[4 * g + 2] = v.z;
        a[4 * g + 3] = v.w;
    }
    return a;
}

// relu of a finished 32 x 32 block to LDS [unit][row]
template <int ROWS>
__device__ __forceinline__ void store_relu(float* s, const f32x16& a, int cb, int rb, int half, int l32) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int unit = 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * half;
        s[unit * ROWS + 32 * rb + l32] = fmaxf(a[r], 0.0f);
    }
}

// The two hidden layers of a tile: s_h1 = relu(W1 s_x + b1), s_h2 = relu(W2 s_h1 + b2), all [unit][ROWS] in LDS.
// s_x holds the 2 S1 input rows (filled and synchronised by the caller); pw1 / pw2 are in the A-operand order of
// rcbf_hip.h.  Every thread of the 256 calls it; it ends after the barrier that makes s_h2 visible.
template <int NRB>
__device__ __forceinline__ void mlp_hidden(const float* s_x, float* s_h1, float* s_h2,
                                           const float* __restrict__ pw1, const float* __restrict__ pb1,
                                           const float* __restrict__ pw2, const float* __restrict__ pb2, int S1,
                                           int H) {
    constexpr int ROWS = 32 * NRB;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, l32 = lane & 31, half = lane >> 5;
    const int S2 = H >> 1, NCB = H >> 5;

    // this wave's unit blocks (wave-uniform; H = 256 gives every wave a pair)
    const int cb0 = 2 * w, cb1 = min(2 * w + 1, NCB - 1);
    const bool work = cb0 < NCB, two = 2 * w + 1 < NCB;

    // layer 1: at most 9 k-steps, one dword of W1 per lane and k-step
    if (work) {
        f32x16 acc[2][NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            acc[0][rb] = bias_acc(pb1, cb0, half);
            acc[1][rb] = bias_acc(pb1, cb1, half);
        }
        for (int s = 0; s < S1; ++s) {
            const float a0 = pw1[(cb0 * S1 + s) * 64 + lane];
            const float a1 = pw1[(cb1 * S1 + s) * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) {
                const float b = s_x[(2 * s + half) * ROWS + 32 * rb + l32];
                acc[0][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][rb], 0, 0, 0);
                acc[1][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][rb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            store_relu<ROWS>(s_h1, acc[0][rb], cb0, rb, half, l32);
            if (two) store_relu<ROWS>(s_h1, acc[1][rb], cb1, rb, half, l32);
        }
    }
    __syncthreads();

    // layer 2: four k-steps of W2 per lane and load (16 B)
    if (work) {
        f32x16 acc[2][NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            acc[0][rb] = bias_acc(pb2, cb0, half);
            acc[1][rb] = bias_acc(pb2, cb1, half);
        }
        const int S4 = S2 >> 2;
        const float4* const q0 = reinterpret_cast<const float4*>(pw2) + (cb0 * S4) * 64 + lane;
        const float4* const q1 = reinterpret_cast<const float4*>(pw2) + (cb1 * S4) * 64 + lane;
        // one load of each block ahead of its use (four ahead measured 12 % slower at every B: DESIGN 5.6);
        // past the end the last group is loaded again
        float4 n0 = q0[0], n1 = q1[0];
        for (int s4 = 0; s4 < S4; ++s4) {
            const float4 c0 = n0, c1 = n1;
            const int nx = min(s4 + 1, S4 - 1);
            n0 = q0[nx * 64];
            n1 = q1[nx * 64];
            const float a0[4] = {c0.x, c0.y, c0.z, c0.w}, a1[4] = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 2 * (4 * s4 + j) + half;
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) {
                    const float b = s_h1[k * ROWS + 32 * rb + l32];
                    acc[0][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b, acc[0][rb], 0, 0, 0);
                    acc[1][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b, acc[1][rb], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) {
            store_relu<ROWS>(s_h2, acc[0][rb], cb0, rb, half, l32);
            if (two) store_relu<ROWS>(s_h2, acc[1][rb], cb1, rb, half, l32);
        }
    }
    __syncthreads();
}

// One output unit of a head for the row on this lane: bias first, k ascending, the MFMA's chain on the VALU
template <int ROWS>
__device__ __forceinline__ float head_chain(const float* __restrict__ wrow, float bias, const float* s_h2, int H,
                                            int row) {
    float a = bias;
#pragma unroll 8
    for (int k = 0; k < H; ++k) a = fmaf(wrow[k], s_h2[k * ROWS + row], a);
    return a;
}

// 0.5 log(2 pi) rounded to fp32 (Normal.log_prob's log(sqrt(2 pi)), model.py:101)
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// The actor's forward of one tile: the body of k_policy_act and rcbf::k_policy_step (rcbf_policy.hip) and, with
// LOGP, of k_actor_sample (rcbf_critic.hip).  LOGP (SAMPLE only) adds GaussianPolicy.sample's two other outputs
// (model.py:101-105), each nullable: u_mean = tanh(mean) * scale + bias, MEAN mode's value, and
//   log_pi = sum_c  ((-0.5 z_c^2 - log_std_c) - 0.5 log(2 pi)) - log(scale_c (1 - y_c^2) + 1e-6)
// with y_c the tanhf value the stored action is formed from, c ascending, every operation rounded on its own.
template <bool SAMPLE, int NRB, bool LOGP = false>
__device__ __forceinline__ void policy_tile(const float* __restrict__ packed, int n_o, int n_u, int H, int64_t B,
                                            const float* __restrict__ obs, float* __restrict__ u_rl,
                                            const float* __restrict__ z, uint64_t seed, uint64_t counter,
                                            int64_t env_offset, float* __restrict__ log_pi = nullptr,
                                            float* __restrict__ u_mean = nullptr) {
    static_assert(SAMPLE || !LOGP, "the log-probability is the sampled action's");
    constexpr int ROWS = 32 * NRB;
    extern __shared__ __align__(16) float pol_smem[];
    float* const s_x = pol_smem;             // [16][ROWS]   obs^T, zero column when n_o is odd
    float* const s_h1 = s_x + 16 * ROWS;     // [H][ROWS]
    float* const s_h2 = s_h1 + H * ROWS;     // [H][ROWS]
    float* const s_hd = s_h2 + H * ROWS;     // [4][ROWS]    head outputs: mean 0..n_u-1, log_std after them

    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int K1 = n_o + (n_o & 1), S1 = K1 >> 1;
    const float* const pw1 = packed;
    const float* const pb1 = pw1 + H * K1;
    const float* const pw2 = pb1 + H;
    const float* const pb2 = pw2 + H * H;
    const float* const pwm = pb2 + H;
    const float* const pbm = pwm + n_u * H;
    const float* const pws = pbm + 4;
    const float* const pbs = pws + n_u * H;
    const float* const pscale = pbs + 4;
    const float* const pbias = pscale + 4;

    // the tile's observations, transposed
    for (int e = t; e < ROWS * n_o; e += 256) {
        const int r = e / n_o, k = e - r * n_o;
        const int64_t gr = row0 + r < B ? row0 + r : B - 1;
        s_x[k * ROWS + r] = obs[gr * n_o + k];
    }
    if ((n_o & 1) && t < ROWS) s_x[n_o * ROWS + t] = 0.0f;
    __syncthreads();

    mlp_hidden<NRB>(s_x, s_h1, s_h2, pw1, pb1, pw2, pb2, S1, H);

    // heads: wave w forms output w (mean 0 .. n_u - 1, then the log_std components when sampling) for the
    // tile's rows, a row per lane, the same chain on the VALU
    const int n_heads = SAMPLE ? 2 * n_u : n_u;
    if (w < n_heads && lane < ROWS) {
        const bool is_mean = w < n_u;
        const int c = is_mean ? w : w - n_u;
        s_hd[w * ROWS + lane] = head_chain<ROWS>((is_mean ? pwm : pws) + c * H, (is_mean ? pbm : pbs)[c], s_h2, H, lane);
    }
    __syncthreads();

    if (t < ROWS * n_u) {
#pragma clang fp contract(off)
        const int c = t / ROWS, r = t - c * ROWS;
        const int64_t gr = row0 + r < B ? row0 + r : B - 1;
        float pre = s_hd[c * ROWS + r];
        [[maybe_unused]] float ls = 0.0f, zz = 0.0f;
        if constexpr (LOGP) {
            if (u_mean && row0 + r < B) u_mean[(row0 + r) * n_u + c] = tanhf(pre) * pscale[c] + pbias[c];
        }
        if constexpr (SAMPLE) {
            ls = fminf(fmaxf(s_hd[(n_u + c) * ROWS + r], -20.0f), 2.0f);
            if (z) {
                zz = z[gr * n_u + c];
            } else {  // the model step's draw (k_model_step, z == NULL): component c of row env_offset + gr
                const uint64_t row = (uint64_t)(env_offset + gr);
                uint32_t cc[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)counter, 0u};
                philox4x32_10(cc, (uint32_t)seed, (uint32_t)(seed >> 32));
                float zc, zs;
                box_muller_pair(cc[0], cc[1], zc, zs);
                zz = c == 0 ? zc : zs;
            }
            pre = pre + expf(ls) * zz;  // normal.rsample(): mean + std * eps (model.py:96-98)
        }
        const float y = tanhf(pre);
        const float u = y * pscale[c] + pbias[c];
        if (row0 + r < B) u_rl[(row0 + r) * n_u + c] = u;
        if constexpr (LOGP) {
            // (x_t - mean)^2 / (2 var) is 0.5 z^2 exactly in real arithmetic; formed from z it has none of the
            // cancellation of x_t - mean.  This thread alone read its two s_hd slots: its term replaces the mean.
            const float normal = (-0.5f * (zz * zz) - ls) - kHalfLog2Pi;
            s_hd[c * ROWS + r] = normal - logf(pscale[c] * (1.0f - y * y) + 1e-6f);
        }
    }
    if constexpr (LOGP) {
        __syncthreads();
        if (log_pi && t < ROWS && row0 + t < B) {
#pragma clang fp contract(off)
            float lp = s_hd[t];
            if (n_u == 2) lp = lp + s_hd[ROWS + t];
            log_pi[row0 + t] = lp;
        }
    }
}

}  // namespace rcbf
