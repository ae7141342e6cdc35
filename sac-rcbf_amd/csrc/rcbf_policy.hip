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
// Two kernel families share the body (policy_tile): k_policy_act, which rcbf_policy_act launches through HIP, and
// rcbf::k_policy_step, which no HIP launch uses: csrc/rcbf_aql.hip dispatches it from librcbf_policy.co, this
// file's gfx950 code object, as the policy packets of a closed-loop plan (rcbf_aql_closed_loop_plan).
#include "rcbf_common.hpp"
#include "rcbf_policy_step.hpp"

using namespace rcbf;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

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

// The forward of one tile: the body of both kernel families (k_policy_act below, rcbf::k_policy_step after the
// anonymous namespace).
template <bool SAMPLE, int NRB>
__device__ __forceinline__ void policy_tile(const float* __restrict__ packed, int n_o, int n_u, int H, int64_t B,
                                            const float* __restrict__ obs, float* __restrict__ u_rl,
                                            const float* __restrict__ z, uint64_t seed, uint64_t counter,
                                            int64_t env_offset) {
    constexpr int ROWS = 32 * NRB;
    extern __shared__ __align__(16) float pol_smem[];
    float* const s_x = pol_smem;             // [16][ROWS]   obs^T, zero column when n_o is odd
    float* const s_h1 = s_x + 16 * ROWS;     // [H][ROWS]
    float* const s_h2 = s_h1 + H * ROWS;     // [H][ROWS]
    float* const s_hd = s_h2 + H * ROWS;     // [4][ROWS]    head outputs: mean 0..n_u-1, log_std after them

    const int t = threadIdx.x, w = t >> 6, lane = t & 63, l32 = lane & 31, half = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int K1 = n_o + (n_o & 1), S1 = K1 >> 1, S2 = H >> 1, NCB = H >> 5;
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

    // this wave's unit blocks (wave-uniform; H = 256 gives every wave a pair)
    const int cb0 = 2 * w, cb1 = min(2 * w + 1, NCB - 1);
    const bool work = cb0 < NCB, two = 2 * w + 1 < NCB;

    // layer 1: K1 <= 16, one dword of W1 per lane and k-step
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

    // heads: wave w forms output w (mean 0 .. n_u - 1, then the log_std components when sampling) for the
    // tile's rows, a row per lane, the same chain on the VALU
    const int n_heads = SAMPLE ? 2 * n_u : n_u;
    if (w < n_heads && lane < ROWS) {
        const bool is_mean = w < n_u;
        const int c = is_mean ? w : w - n_u;
        const float* const wrow = (is_mean ? pwm : pws) + c * H;
        float a = (is_mean ? pbm : pbs)[c];
#pragma unroll 8
        for (int k = 0; k < H; ++k) a = fmaf(wrow[k], s_h2[k * ROWS + lane], a);
        s_hd[w * ROWS + lane] = a;
    }
    __syncthreads();

    if (t < ROWS * n_u) {
#pragma clang fp contract(off)
        const int c = t / ROWS, r = t - c * ROWS;
        const int64_t gr = row0 + r < B ? row0 + r : B - 1;
        float pre = s_hd[c * ROWS + r];
        if constexpr (SAMPLE) {
            const float ls = fminf(fmaxf(s_hd[(n_u + c) * ROWS + r], -20.0f), 2.0f);
            float zz;
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
        const float u = tanhf(pre) * pscale[c] + pbias[c];
        if (row0 + r < B) u_rl[(row0 + r) * n_u + c] = u;
    }
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
