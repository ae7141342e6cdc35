// rcbf_safe_step.hpp -- the fused safe step kernel (the hot path bench.py
// measures) and the env-state / observation memory helpers it shares with
// the env kernels.  Included by rcbf_env.hip (the product instantiation) and
// by csrc/study/rcbf_stamps.hip (the phase-timing study build).
//
// Env state is component-PAIR-major in HBM (see rcbf_common.hpp): one env per
// lane, each lane moves 16 B per component pair, and a wavefront's load or
// store of one pair is one contiguous 1 KiB access (dwordx4).  The fused step
// reads x, t, step, u_RL and writes x', t', step', obs (AoS, the policy's
// (B, n_o) input), u, reward, cost, done; the episode counter is touched only
// on resets.
#pragma once

#include <cstddef>

#include "rcbf_common.hpp"

// study override: prefetch this many argument lines in every mode
#ifndef RCBF_KARG_PREFETCH
#define RCBF_KARG_PREFETCH 0
#endif
// 1: the cars step stores the state pairs that do not depend on the safe
// action before the layer's chain runs (k_safe_step; 3.86 -> 3.67 us per
// step, profiles/r03/early_store_confirm_r03k.txt); 0: after it
#ifndef RCBF_EARLY_STORE
#define RCBF_EARLY_STORE 1
#endif

namespace rcbf {

// Touch each 64-B line of the first NL lines of the kernel argument block
// once, right after the state loads are issued, so the scalar loads of the
// parameters the compiler sinks into the body hit the scalar cache instead
// of each waiting for a miss on the critical path.  The global loads stay in
// flight across the one wait here.
template <int NL>
__device__ __forceinline__ void prefetch_kernargs() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t* ka = (const uint32_t*)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t acc = 0;
#pragma unroll
    for (int l = 0; l < NL; ++l) acc ^= ka[16 * l];
    asm volatile("" ::"s"(acc));
    __builtin_amdgcn_sched_barrier(0);
#endif
}

template <int MODE>
__device__ __forceinline__ void load_state(const double* x, int64_t B, int64_t i, double* xs) {
    constexpr int NS = Dims<MODE, 1>::NS;
#pragma unroll
    for (int p = 0; p < NS / 2; ++p) {
        double2 v = ld_in2(&x[2 * (p * B + i)]);
        xs[2 * p] = v.x;
        xs[2 * p + 1] = v.y;
    }
    if constexpr (NS % 2) xs[NS - 1] = ld_in(&x[(NS - 1) * B + i]);
}

template <int MODE, typename XP = double*>  // XP: double* or gptr<double>
__device__ __forceinline__ void store_state(XP x, int64_t B, int64_t i, const double* xs) {
    constexpr int NS = Dims<MODE, 1>::NS;
#pragma unroll
    for (int p = 0; p < NS / 2; ++p) st_out2d(&x[2 * (p * B + i)], xs[2 * p], xs[2 * p + 1]);
    if constexpr (NS % 2) st_out(&x[(NS - 1) * B + i], xs[NS - 1]);
}

// OP (here and below): float* or gptr<float>
template <int MODE, bool WT = false, typename OP = float*>
__device__ __forceinline__ void store_obs32(OP obs, int64_t i, const double* xs,
                                            const double* obs_cache = nullptr) {
    constexpr int NO = Dims<MODE, 1>::NO;
    double o[NO];
    if constexpr (MODE == RCBF_MODE_UNICYCLE) {
        if (obs_cache && obs_cache[3] != 0.0)
            uni_obs_cs(xs, obs_cache[0], obs_cache[1], obs_cache[2], o);
        else
            env_obs<MODE>(xs, o);
    } else {
        env_obs<MODE>(xs, o);
    }
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
        const OP ov = obs + i * NO;  // 40 B rows, 8 B aligned
#pragma unroll
        for (int k = 0; k < NO / 2; ++k) {
            if constexpr (WT) {
                const float pr[2] = {(float)o[2 * k], (float)o[2 * k + 1]};
                uint64_t w;
                __builtin_memcpy(&w, pr, 8);
                st_wt(reinterpret_cast<uint64_t*>(ov + 2 * k), w);
            } else {
                st_out2(ov + 2 * k, (float)o[2 * k], (float)o[2 * k + 1]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < NO; ++k) st_any<WT>(&obs[i * NO + k], (float)o[k]);
    }
}

// The wave's staged observation block (64 rows in LDS) to HBM as 16-byte
// chunks, chunk c by lane c % 64.  Every chunk is read from LDS first, then
// stored: the write-through store is an asm with a memory clobber, which
// would otherwise hold each following LDS read (and its wait) behind the
// previous store.  SC1: the chunks leave write-through (st_out4).
template <int MODE, bool WT = false, bool SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS, typename OP = float*>
__device__ __forceinline__ void store_obs_chunks(OP obs, int64_t base, const float* lds_wave, int lane) {
    constexpr int NO = Dims<MODE, 1>::NO;
    __builtin_amdgcn_wave_barrier();
    constexpr int CH = NO * 16;  // 16-byte chunks in the wave's block
    const float4* src = reinterpret_cast<const float4*>(lds_wave);
    const OP dst = obs + base * NO;
    constexpr int NJ = (CH + 63) / 64;
    float4 chunk[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        if (CH % 64 == 0 || c < CH) chunk[j] = src[c];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        if (CH % 64 == 0 || c < CH) st_out4<SC1>(dst + 4 * c, chunk[j]);
    }
}

// Observation store through LDS: a full wave's 64 obs rows are one
// contiguous (64*NO*4)-byte block; lanes write their rows into LDS, then
// store the block as 16-byte chunks, chunk c by lane c%64 -- every store
// instruction covers whole contiguous lines (cars: 3 dwordx4 instead of 5
// strided dwordx2).  Partial or unaligned waves take the per-lane path.
template <int MODE, bool WT = false, bool SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS, typename OP = float*>
__device__ __forceinline__ void store_obs32_staged(OP obs, int64_t i, int64_t B, const double* xs,
                                                   const double* obs_cache, float* lds_wave, int lane) {
    constexpr int NO = Dims<MODE, 1>::NO;
    const int64_t base = i - lane;
#ifdef RCBF_STUDY_EPW  // study: a 64-thread workgroup's wave holds fewer than 64 envs (per-lane stores)
    const bool full = blockDim.x != 64 && (base + 64 <= B) && ((reinterpret_cast<uintptr_t>(obs) & 15) == 0);
#else
    const bool full = (base + 64 <= B) && ((reinterpret_cast<uintptr_t>(obs) & 15) == 0);
#endif
    if (!full) {
        store_obs32<MODE, WT>(obs, i, xs, obs_cache);
        return;
    }
    double o[NO];
    if constexpr (MODE == RCBF_MODE_UNICYCLE) {
        if (obs_cache && obs_cache[3] != 0.0)
            uni_obs_cs(xs, obs_cache[0], obs_cache[1], obs_cache[2], o);
        else
            env_obs<MODE>(xs, o);
    } else {
        env_obs<MODE>(xs, o);
    }
    if constexpr (NO % 2 == 0) {
#pragma unroll
        for (int k = 0; k < NO / 2; ++k)
            *reinterpret_cast<float2*>(&lds_wave[lane * NO + 2 * k]) = make_float2((float)o[2 * k], (float)o[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < NO; ++k) lds_wave[lane * NO + k] = (float)o[k];
    }
    store_obs_chunks<MODE, WT, SC1>(obs, base, lds_wave, lane);
}

// One fused safe step of env i, from its state and inputs in registers (xs, a,
// st, us, m, s; ep_pre / ep0: the episode counter loaded ahead, see
// reset_foreseeable) to every store a step makes: the state pairs, aux, step,
// the episode counter on a reset, the observation (staged through obs_stage,
// this wave's 64 x NO floats of LDS; lane: threadIdx.x & 63), u, reward, cost, done, goal_met, the
// status and the fail_flag OR.  xs, a and st come back as the post-step state,
// *did_reset (if asked for) whether the step reset the env.
// Shared by k_safe_step (one step per dispatch) and k_safe_steps (K steps per
// dispatch): one source for both.  wt_lds: the write-through staging block of
// the RCBF_WT_OUT study build.  GP: the buffers come as gptr (k_safe_steps), so every access is a global_*
// instruction by type; k_safe_step passes its kernel arguments as they are.  OBS_SC1: the staged observation
// chunks' store flavour (st_out4).
template <int SOLVER, int MODE, int K, bool ST, bool WT, bool GP = false,
          bool OBS_SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS>
__device__ __forceinline__ void safe_step_body(
    const rcbf_params& prm, int64_t B, int64_t i, ptr_g<GP, double> __restrict__ x, ptr_g<GP, double> __restrict__ aux,
    ptr_g<GP, int32_t> __restrict__ step, ptr_g<GP, uint32_t> __restrict__ episode,
    ptr_g<GP, float> __restrict__ obs_out, ptr_g<GP, float> __restrict__ u_out, ptr_g<GP, float> __restrict__ reward,
    ptr_g<GP, float> __restrict__ cost, ptr_g<GP, uint8_t> __restrict__ done, ptr_g<GP, uint8_t> __restrict__ goal_met,
    ptr_g<GP, int32_t> __restrict__ status_out, ptr_g<GP, int32_t> fail_flag, int auto_reset,
    uint64_t seed, int64_t off, double* xs, double& a, int& st, const float* us, const float* m, const float* s,
    bool ep_pre, uint32_t ep0, const Stamps<ST>& stamps, float* obs_stage, char* wt_lds, int lane,
    bool* did_reset = nullptr) {
    using D = Dims<MODE, K>;
    const int64_t wbase = i - lane;
    const bool wfull = wbase + 64 <= B;  // wave-uniform: every lane of this wave is live
    constexpr int kWtBytes = WT ? 16 * 160 : 16;  // the caller's per-wave wt_lds block
    (void)wt_lds;
    (void)wfull;
    (void)kWtBytes;
    float rew, cst;
    bool dn, gm;
    int status;
    float uf[D::NU];
    double oc[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS && RCBF_EARLY_STORE && !ST) {
        // The same step in an order that lets 76 of the 145 written bytes
        // leave while the layer's chain is still running: the env's
        // pre-step part (everything but car 3's velocity, t, step, done,
        // cost) and the auto-reset do not depend on the safe action, so
        // they, and the stores of state pairs 0, 1, 2, 4, t and step, come
        // first; the layer's chain (state32 -> rows -> QP -> clamp) then
        // finishes car 3's velocity (pair 3) and the observation.
        float s32[D::NS];
        state_from_env<MODE>(xs, s32);  // the layer reads the pre-step state
        // the exact solver on the raw rows: the rows are built here, ahead of
        // the env's pre-step part, whose arithmetic can then fill their latency
        // (3.69 -> 3.65 us per step, profiles/r03/rows_first_ab_r03q.txt)
        constexpr bool kRowsFirst = SOLVER == RCBF_SOLVER_ACTIVE_SET && RCBF_FUSED_RAW_ROWS != 0;
        LayerState<MODE, K> L;
        if constexpr (kRowsFirst) diff_rows<MODE, K>(prm, s32, us, m, s, L.G, L.h, nullptr);
        CarsStepOut o;
        const double acc3 = cars_env_pre(prm, xs, a, st, o);
        dn = o.done;
        cst = (float)o.cost;
        gm = false;
        const bool rs = auto_reset && dn;
        if (rs) {
            const uint32_t ep = episode ? (ep_pre ? ep0 : episode[i]) + 1u : 0u;
            if (episode) {
                if constexpr (WT)
                    st_wt(&episode[i], ep);
                else
                    episode[i] = ep;
            }
            env_reset_one<MODE>(nullptr, i, seed, off, ep, xs, a, st);
        }
#pragma unroll
        for (int p = 0; p < D::NS / 2; ++p)
            if (p != 3) st_any2d<WT>(&x[2 * (p * B + i)], xs[2 * p], xs[2 * p + 1]);
        if constexpr (WT) {
            using E = WtStage<8, 4>;  // aux, step
            char* const dst[2] = {reinterpret_cast<char*>(aux + wbase), reinterpret_cast<char*>(step + wbase)};
            const uint64_t val[2] = {wt_bits(a), wt_bits(st)};
            E::store(wt_lds, lane, wfull, dst, val);
        } else {
            st_out(&aux[i], a);
            st_out(&step[i], st);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the early stores ahead of the layer's chain
        if constexpr (kRowsFirst) {
            layer_solve_raw<MODE, K>(prm, us, uf, L);  // the same solve as layer_forward<..., RAW>
        } else {
            layer_forward<SOLVER, MODE, K, false, false, RCBF_FUSED_RAW_ROWS != 0>(prm, s32, us, m, s, uf, L);
        }
        status = L.qp.status;
        const double v3_reset = xs[7];
        cars_env_post<float>(xs, acc3, uf[0], o);  // car 3's velocity and the reward
        xs[7] = rs ? v3_reset : xs[7];
        rew = o.reward;
        st_any2d<WT>(&x[2 * (3 * B + i)], xs[6], xs[7]);
    } else {
        safe_step_one<SOLVER, MODE, K, ST, WT>(prm, i, xs, a, st, episode, us, m, s, uf, rew, cst, dn, gm, status,
                                               auto_reset, seed, off, stamps, oc, ep_pre, ep0);
        if constexpr (WT) {
#pragma unroll
            for (int p = 0; p < D::NS / 2; ++p) st_wt2d(&x[2 * (p * B + i)], xs[2 * p], xs[2 * p + 1]);
            // the odd component (unicycle theta), aux and step leave with the outputs below
        } else {
            store_state<MODE>(x, B, i, xs);
            st_out(&aux[i], a);
            st_out(&step[i], st);
        }
    }
    store_obs32_staged<MODE, WT, OBS_SC1>(obs_out, i, B, xs, oc, obs_stage, lane);
    if constexpr (WT) {
        constexpr int NU4 = 4 * D::NU;
        float ufc[D::NU];
#pragma unroll
        for (int c = 0; c < D::NU; ++c) ufc[c] = uf[c];
        char* const u_d = reinterpret_cast<char*>(u_out + wbase * D::NU);
        char* const r_d = reinterpret_cast<char*>(reward + wbase);
        char* const c_d = reinterpret_cast<char*>(cost + wbase);
        char* const d_d = reinterpret_cast<char*>(done + wbase);
        uint64_t u_v = 0;
        __builtin_memcpy(&u_v, ufc, sizeof(ufc));
        const uint64_t r_v = wt_bits(rew), c_v = wt_bits(cst), d_v = (uint64_t)dn;
        if constexpr (MODE == RCBF_MODE_SIMULATED_CARS && RCBF_EARLY_STORE) {
            if (goal_met) {
                using E = WtStage<NU4, 4, 4, 1, 1>;
                char* const dst[5] = {u_d, r_d, c_d, d_d, reinterpret_cast<char*>(goal_met + wbase)};
                const uint64_t val[5] = {u_v, r_v, c_v, d_v, (uint64_t)gm};
                E::store(wt_lds, lane, wfull, dst, val);
            } else {
                using E = WtStage<NU4, 4, 4, 1>;
                char* const dst[4] = {u_d, r_d, c_d, d_d};
                const uint64_t val[4] = {u_v, r_v, c_v, d_v};
                E::store(wt_lds, lane, wfull, dst, val);
            }
        } else {
            static_assert(D::NS % 2 == 1, "the late write-through block carries the odd state component");
            char* const x_d = reinterpret_cast<char*>(x + (D::NS - 1) * B + wbase);
            char* const a_d = reinterpret_cast<char*>(aux + wbase);
            char* const s_d = reinterpret_cast<char*>(step + wbase);
            const uint64_t x_v = wt_bits(xs[D::NS - 1]), a_v = wt_bits(a), s_v = wt_bits(st);
            if (goal_met) {
                using E = WtStage<8, 8, 4, NU4, 4, 4, 1, 1>;
                static_assert(E::kBytes <= kWtBytes, "wt_lds");
                char* const dst[8] = {x_d, a_d, s_d, u_d, r_d, c_d, d_d, reinterpret_cast<char*>(goal_met + wbase)};
                const uint64_t val[8] = {x_v, a_v, s_v, u_v, r_v, c_v, d_v, (uint64_t)gm};
                E::store(wt_lds, lane, wfull, dst, val);
            } else {
                using E = WtStage<8, 8, 4, NU4, 4, 4, 1>;
                char* const dst[7] = {x_d, a_d, s_d, u_d, r_d, c_d, d_d};
                const uint64_t val[7] = {x_v, a_v, s_v, u_v, r_v, c_v, d_v};
                E::store(wt_lds, lane, wfull, dst, val);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < D::NU; ++c) st_out(&u_out[i * D::NU + c], uf[c]);
        st_out(&reward[i], rew);
        st_out(&cost[i], cst);
        st_out(&done[i], (uint8_t)dn);
        if (goal_met) st_out(&goal_met[i], (uint8_t)gm);
    }
    if (did_reset) *did_reset = auto_reset && dn;  // the condition under which the step above reset the env
    stamps.mark(6, false);
    if constexpr (WT) {
        if (status_out) st_wt(&status_out[i], (int32_t)status);
        if (status != RCBF_QP_OK && fail_flag) atomicOr(fail_flag, 1 << status);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing this wave wrote is in flight when it ends
    } else {
        report(status, status_out, i, fail_flag);
    }
}

// The fused safe step (rcbf_safe_step): one env per lane.  ST = true only in
// the study build (csrc/study/rcbf_stamps.hip), which records phase
// timestamps into `stamps`; the product instantiation ignores it.
// BS: workgroup size (block_for_envs).  SPAN = true (rcbf_safe_step_span, a
// measurement entry point of the product library): lane 0 of every wave
// writes the chip clock (s_memrealtime, 100 MHz) at its start and after its
// own stores have completed to stamp_buf[4 w], [4 w + 1], and the shader
// clock (s_memtime) at the same two points to stamp_buf[4 w + 2], [4 w + 3]
// (the clock the wave ran at is delta(s_memtime) / delta(s_memrealtime) x
// 100 MHz); every other instruction is the product's.
// Argument order: B and the pointers of the first loads lead (one 64-B line
// of the argument block, which the launch can preload into SGPRs), the
// parameter block comes last.
template <int SOLVER, int MODE, int K, bool ST = false, int BS = kBlock, bool SPAN = false>
__global__ void __launch_bounds__(BS) k_safe_step(int64_t B, double* __restrict__ x, double* __restrict__ aux,
                                                      int32_t* __restrict__ step, const float* __restrict__ u_rl,
                                                      uint32_t* __restrict__ episode, const float* __restrict__ mu,
                                                      const float* __restrict__ sigma, float* __restrict__ obs_out,
                                                      float* __restrict__ u_out, float* __restrict__ reward,
                                                      float* __restrict__ cost, uint8_t* __restrict__ done,
                                                      uint8_t* __restrict__ goal_met,
                                                      int32_t* __restrict__ status_out, int32_t* fail_flag,
                                                      int auto_reset, uint64_t seed, int64_t off, rcbf_params prm,
                                                      int prior_cols = 0, unsigned long long* stamp_buf = nullptr) {
    using D = Dims<MODE, K>;
    // RCBF_WT_OUT: every output write-through, the wave's stores drained before
    // it ends (rcbf_common.hpp, WtStage); the study stamps build keeps the nt form
    constexpr bool WT = RCBF_WT_OUT != 0 && !ST;
    int64_t i = env_index<BS>();
    if (i >= B) return;
    constexpr int kWtBytes = WT ? 16 * 160 : 16;  // per wave: the largest WtStage of the body (unicycle, 152 chunks)
    __shared__ __attribute__((aligned(16))) char wt_lds_all[BS / 64][kWtBytes];
    char* wt_lds = wt_lds_all[threadIdx.x >> 6];
    unsigned long long span_t0 = 0, span_c0 = 0;
    if constexpr (SPAN) {
        span_t0 = __builtin_amdgcn_s_memrealtime();
        span_c0 = __builtin_amdgcn_s_memtime();
    }
    Stamps<ST> stamps;
    stamps.buf = stamp_buf;
    stamps.mark(0, false);
    double xs[D::NS];
    load_state<MODE>(x, B, i, xs);
    double a = ld_in(&aux[i]);
    int st = ld_in(&step[i]);
    float us[D::NU], m[D::NS], s[D::NS];
#pragma unroll
    for (int c = 0; c < D::NU; ++c) us[c] = ld_in(&u_rl[i * D::NU + c]);
#if RCBF_KARG_PREFETCH
    prefetch_kernargs<RCBF_KARG_PREFETCH>();
#else
    // cars: 3.87 -> 3.81 us per step; the unicycle step is slower with it
    // (4.38 -> 4.50 us at k = 5; profiles/r03/kernarg_preload_ab_r03d.txt)
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) prefetch_kernargs<7>();
#endif
    const bool ep_pre = episode && reset_foreseeable<MODE>(st, a);
    uint32_t ep0 = 0;
    if (ep_pre) ep0 = episode[i];
    if (prior_cols) {
        // column layout (rcbf_safe_step_cols): only what the rows read, one
        // contiguous (B,) f32 column each -- cars sigma (3, B) = sigma[:, 5],
        // [:, 7], [:, 9] (the cars rows ignore mu, diff_cbf_qp.py:298-299);
        // unicycle mu and sigma (3, B)
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = 0.0f;
            s[k] = prior_sigma<MODE>(k);
        }
        if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
            if (sigma) {
                s[5] = ld_in(&sigma[i]);
                s[7] = ld_in(&sigma[B + i]);
                s[9] = ld_in(&sigma[2 * B + i]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < D::NS; ++k) {
                if (mu) m[k] = ld_in(&mu[k * B + i]);
                if (sigma) s[k] = ld_in(&sigma[k * B + i]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = mu ? mu[i * D::NS + k] : 0.0f;
            s[k] = sigma ? sigma[i * D::NS + k] : prior_sigma<MODE>(k);
        }
    }
    stamps.mark(1, true);
    __shared__ float obs_stage[BS / 64][64 * D::NO];
    safe_step_body<SOLVER, MODE, K, ST, WT>(prm, B, i, x, aux, step, episode, obs_out, u_out, reward, cost, done,
                                            goal_met, status_out, fail_flag, auto_reset, seed, off, xs, a, st, us, m,
                                            s, ep_pre, ep0, stamps, obs_stage[threadIdx.x >> 6], wt_lds,
                                            threadIdx.x & 63);
    stamps.mark(7, true);
    if constexpr (SPAN) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have landed
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long c1 = __builtin_amdgcn_s_memtime();
        if ((threadIdx.x & 63) == 0) {
            const int64_t w = ((int64_t)blockIdx.x * BS + threadIdx.x) >> 6;
            typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u2*>(stamp_buf + 4 * w) = u2{span_t0, t1};
            *reinterpret_cast<u2*>(stamp_buf + 4 * w + 2) = u2{span_c0, c1};
        }
    }
}

// k_safe_steps: which kernels keep their loop's values in plain variables (true) and which behind opaque
// copies in accumulation registers (false; see the kernel): plain wherever the kernel then has no scalar or
// vector spill and no scratch (tests/test_abi_fused_cpu.py).  Cars fits (168 VGPRs, 106 SGPRs) and so does
// the unicycle at k = 1; written plain, the unicycle at k = 2, 3, 4, 5, 6 spills 2, 6, 8, 12, 8 scalar
// registers (256-thread workgroups).
template <int MODE, int K>
constexpr bool fused_plain() {
    return MODE == RCBF_MODE_SIMULATED_CARS || K == 1;
}

// Argument block of k_safe_steps, at the offsets of its parameter list (the
// AMDGPU kernarg ABI: every argument at its natural alignment): k_safe_step's
// block with the u_RL table in u_rl's place and n_u, steps, ju0 in the stamp
// pointer's.  The plan builder (csrc/rcbf_aql.hip) writes it; rcbf_aql_open and
// tests/test_abi_fused_cpu.py check it against the code object.
struct SafeStepsArgs {
    int64_t B;
    double* x;
    double* aux;
    int32_t* step;
    const float* const* u_tab;
    uint32_t* episode;
    const float* mu;
    const float* sigma;
    float* obs_out;
    float* u_out;
    float* reward;
    float* cost;
    uint8_t* done;
    uint8_t* goal_met;
    int32_t* status_out;
    int32_t* fail_flag;
    int32_t auto_reset;
    uint64_t seed;
    int64_t off;
    rcbf_params prm;
    int32_t prior_cols;
    int32_t n_u;
    int32_t steps;
    int32_t ju0;
};
static_assert(offsetof(SafeStepsArgs, auto_reset) == 128 && offsetof(SafeStepsArgs, seed) == 136 &&
                  offsetof(SafeStepsArgs, prm) == 152 && offsetof(SafeStepsArgs, prior_cols) == 392 &&
                  offsetof(SafeStepsArgs, n_u) == 396 && offsetof(SafeStepsArgs, steps) == 400 &&
                  offsetof(SafeStepsArgs, ju0) == 404 && sizeof(SafeStepsArgs) == 408,
              "kernarg layout");

// K consecutive fused safe steps of a plan in ONE dispatch (the fused form of
// rcbf_aql_safe_step_plan): the lane that owns env i runs all `steps` steps of
// env i.  Env i at step j + 1 reads only what env i wrote at step j, its own
// u_RL element and the priors, so no step needs anything another lane, wave or
// XCD produced, and neither the fence between two dispatches nor the re-load
// of x, aux, step is needed.  Every step still makes every store a k_safe_step
// dispatch makes (safe_step_body), so after the dispatch HBM holds what
// `steps` dispatches leave.  Step j reads u_tab[(ju0 + j) % n_u]: u_tab is a
// table of n_u device pointers in device memory, ju0 < n_u.  The u_RL buffers
// must not overlap anything the steps write (the next step's action is loaded
// before this step's stores; the plan builder checks it).  Same grid,
// workgroup size and lane-to-env map as k_safe_step; the exact solver only.
// The argument block (SafeStepsArgs above) keeps k_safe_step's offsets, with
// the table in u_rl's place.
template <int MODE, int K, int BS = kBlock>
__global__ void __launch_bounds__(BS) k_safe_steps(int64_t B, double* __restrict__ x, double* __restrict__ aux,
                                                       int32_t* __restrict__ step,
                                                       const float* const* __restrict__ u_tab,
                                                       uint32_t* __restrict__ episode, const float* __restrict__ mu,
                                                       const float* __restrict__ sigma, float* __restrict__ obs_out,
                                                       float* __restrict__ u_out, float* __restrict__ reward,
                                                       float* __restrict__ cost, uint8_t* __restrict__ done,
                                                       uint8_t* __restrict__ goal_met,
                                                       int32_t* __restrict__ status_out, int32_t* fail_flag,
                                                       int auto_reset, uint64_t seed, int64_t off, rcbf_params prm,
                                                       int prior_cols, int n_u, int steps, int ju0) {
    using D = Dims<MODE, K>;
    constexpr int SOLVER = RCBF_SOLVER_ACTIVE_SET;
    constexpr bool WT = false;
    constexpr bool PLAIN = fused_plain<MODE, K>();
    // the staged observation chunks leave `nt` here, cars included: no kernel end follows a step, the next
    // step rewrites the line, and `sc1` would write each step's chunks through to HBM (measured: DESIGN 5.2)
    constexpr bool OBS_SC1 = false;
    int64_t i = env_index<BS>();
    if (i >= B) return;
    double xs[D::NS];
    load_state<MODE>(x, B, i, xs);
    double a = ld_in(&aux[i]);
    int st = ld_in(&step[i]);
    // The u_RL table, read with scalar loads: its address, ju0, n_u and steps are the same for every lane,
    // and nothing writes it while a plan runs, which its type says (the constant address space: a uniform
    // load from it is a scalar load wherever it stands among the loop's stores).  Its entries are addresses
    // of global memory, and are typed so (gptr, rcbf_common.hpp).
    typedef const uint64_t __attribute__((address_space(4)))* ctab_t;
    const ctab_t tab = (ctab_t)reinterpret_cast<const uint64_t*>(u_tab);
    float us[D::NU], m[D::NS], s[D::NS];
    {
        const gptr<const float> u0 = reinterpret_cast<gptr<const float>>(tab[ju0]);
#pragma unroll
        for (int c = 0; c < D::NU; ++c) us[c] = ld_in(&u0[i * D::NU + c]);
    }
    // env i's episode counter, which only this lane writes (at a reset): read once, then kept in a register
    uint32_t epr = episode ? ld_in(&episode[i]) : 0u;
    // step 1's buffer: every step issues the load of the next step's action from an address that the step
    // before it fetched, so neither the table entry nor the action is ever waited for where it is asked for
    int ju = ju0 + 1 == n_u ? 0 : ju0 + 1;
    gptr<const float> u_next = reinterpret_cast<gptr<const float>>(tab[ju]);
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) prefetch_kernargs<7>();
    // the priors: inputs of the plan that nothing in a run writes, loaded once (k_safe_step's layouts)
    if (prior_cols) {
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = 0.0f;
            s[k] = prior_sigma<MODE>(k);
        }
        if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
            if (sigma) {
                s[5] = ld_in(&sigma[i]);
                s[7] = ld_in(&sigma[B + i]);
                s[9] = ld_in(&sigma[2 * B + i]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < D::NS; ++k) {
                if (mu) m[k] = ld_in(&mu[k * B + i]);
                if (sigma) s[k] = ld_in(&sigma[k * B + i]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = mu ? mu[i * D::NS + k] : 0.0f;
            s[k] = sigma ? sigma[i * D::NS + k] : prior_sigma<MODE>(k);
        }
    }
    __shared__ float obs_stage[BS / 64][64 * D::NO];
    // k = 8 only: the parameter block, one copy per wave, written by every live lane of the wave (the same
    // values; a wave's LDS operations execute in order, so its reads below see them)
    __shared__ rcbf_params prm_stage[K >= 8 ? BS / 64 : 1];
    if constexpr (K >= 8) {
        prm_stage[threadIdx.x >> 6] = prm;
        __builtin_amdgcn_wave_barrier();
    }
    const Stamps<false> stamps{};
    // Register budget of the loop.  Whatever the body derives from loop-invariant values alone (null
    // tests and per-lane addresses of the 15 buffers, the 60 dwords of the parameter block, the loop's
    // own counters) the compiler hoists out of the loop, where it stays live over the whole body on top
    // of what one step needs.  Where that fits (PLAIN, fused_plain above) the loop is written as it reads.
    // The unicycle step alone takes every scalar register there is, and at 7 and 8 hazards every vector
    // register: there everything the loop carries beside the env's state lives in accumulation registers
    // (the unified file has room), as uniform per-lane values behind empty asm copies the compiler cannot
    // see through; no instruction is emitted for a copy, a use costs one register read.  Every step then
    // derives from them what k_safe_step derives once per dispatch, and the parameter block is read from
    // the argument segment again (scalar loads that hit the scalar cache; vector loads at k = 8).  The
    // walk of the table stays scalar: the wave-uniform values are read back with readfirstlane.  In both
    // forms the buffers are gptr, so every access is a global_* instruction.  No kernel spills.
    int64_t Bv = B;
    gptr<double> xv = (gptr<double>)x;
    gptr<double> auxv = (gptr<double>)aux;
    gptr<int32_t> stepv = (gptr<int32_t>)step;
    gptr<uint32_t> epv = (gptr<uint32_t>)episode;
    gptr<float> obsv = (gptr<float>)obs_out;
    gptr<float> uv = (gptr<float>)u_out;
    gptr<float> rewv = (gptr<float>)reward;
    gptr<float> costv = (gptr<float>)cost;
    gptr<uint8_t> donev = (gptr<uint8_t>)done;
    gptr<uint8_t> goalv = (gptr<uint8_t>)goal_met;
    gptr<int32_t> statv = (gptr<int32_t>)status_out;
    gptr<int32_t> failv = (gptr<int32_t>)fail_flag;
    uint64_t tabv = reinterpret_cast<uint64_t>(u_tab), unextv = reinterpret_cast<uint64_t>(u_next);
    int arv = auto_reset, lanev = threadIdx.x & 63, nuv = n_u, juv = ju, leftv = steps,
        widv = threadIdx.x >> 6;
    uint64_t seedv = seed;
    int64_t offv = off;
#define RCBF_OPAQUE_V()                                                                                          \
    if constexpr (!PLAIN) {                                                                                      \
        asm volatile("" : "+a"(xv), "+a"(auxv), "+a"(stepv), "+a"(epv), "+a"(obsv), "+a"(uv), "+a"(rewv));     \
        asm volatile("" : "+a"(costv), "+a"(donev), "+a"(goalv), "+a"(statv), "+a"(failv), "+a"(epr),         \
                     "+a"(Bv), "+a"(arv), "+a"(lanev), "+a"(i));                                                 \
        asm volatile("" : "+a"(widv), "+a"(tabv), "+a"(nuv), "+a"(juv), "+a"(leftv), "+a"(seedv), "+a"(offv),   \
                     "+a"(unextv));                                                                              \
    }
    RCBF_OPAQUE_V();  // once: uniform values, kept in accumulation registers from here on
    // Everything loaded so far has arrived before the loop is entered (vmcnt(0); expcnt and lgkmcnt left
    // alone).  A wait for one of these loads inside the loop would be passed again in every step, where all
    // it can wait for is the last step's stores.
    __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma nounroll
    while (leftv > 0) {
        RCBF_OPAQUE_V();  // every step: nothing derived from them is loop-invariant to the compiler
        const rcbf_params* prm_p = &prm;
        if constexpr (!PLAIN) {
#pragma unroll
            for (int k = 0; k < D::NS; ++k) asm volatile("" : "+a"(m[k]), "+a"(s[k]));  // the priors too
            if constexpr (K >= 8) {
                // k = 8: the step's scalar registers are all taken, so its parameters are read per lane, from
                // this wave's copy in LDS (prm_stage; behind a per-lane zero the compiler cannot see through,
                // which keeps the LDS provenance: ds_read).  Vector loads from the argument segment would count
                // in vmcnt behind the last step's stores, and waiting for them would wait for those.
                uint32_t prm_voff = 0;
                asm volatile("" : "+v"(prm_voff));
                prm_p = reinterpret_cast<const rcbf_params*>(reinterpret_cast<const char*>(&prm_stage[widv]) +
                                                             prm_voff);
            } else {
                uint32_t prm_off = 0;
                asm volatile("" : "+s"(prm_off));
                prm_p = reinterpret_cast<const rcbf_params*>(reinterpret_cast<const char*>(&prm) + prm_off);
            }
        }
        const rcbf_params& prm_j = *prm_p;
        // the next step's action, issued ahead of this step's chain from the address the last step fetched
        float un[D::NU];
#pragma unroll
        for (int c = 0; c < D::NU; ++c) un[c] = 0.0f;
        --leftv;
        if (leftv > 0) {
            const gptr<const float> u1 = reinterpret_cast<gptr<const float>>(unextv);
#pragma unroll
            for (int c = 0; c < D::NU; ++c) un[c] = ld_in(&u1[i * D::NU + c]);
        }
        // the address of the buffer of the step after the next: a scalar load (an entry of the table whether
        // or not that step runs), whose result is first needed at the end of this step
        uint64_t unext2;
        {
            int nu_s = n_u, ju_s = juv;
            uint64_t tab_s = reinterpret_cast<uint64_t>(u_tab);
            if constexpr (!PLAIN) {
                // out of their accumulation registers, as the wave-uniform values they are
                tab_s = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(tabv >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tabv);
                nu_s = __builtin_amdgcn_readfirstlane(nuv);
                ju_s = __builtin_amdgcn_readfirstlane(juv);
            }
            ju_s = ju_s + 1 == nu_s ? 0 : ju_s + 1;
            juv = ju_s;
            unext2 = reinterpret_cast<ctab_t>(tab_s)[ju_s];
        }
        bool rs = false;
        safe_step_body<SOLVER, MODE, K, false, WT, true, OBS_SC1>(prm_j, Bv, i, xv, auxv, stepv, epv, obsv, uv, rewv,
                                                                  costv, donev, goalv, statv, failv, arv, seedv, offv,
                                                                  xs, a, st, us, m, s, epv != nullptr, epr, stamps,
                                                                  obs_stage[widv], nullptr, lanev, &rs);
        epr += rs ? 1u : 0u;  // a reset stored epr + 1
        // this step's chunk reads of obs_stage stay ahead of the next step's writes to it (one wave's LDS
        // operations execute in order; this keeps the compiler from reordering them)
        __builtin_amdgcn_wave_barrier();
        // every step's stores are made in that step: without this the compiler, which sees in the plain form
        // that a step overwrites what the last one stored to aux, step, u, reward, cost and done, keeps those
        // in registers and stores them once after the loop (no instruction, no wait: a compiler barrier)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int c = 0; c < D::NU; ++c) us[c] = un[c];
        if constexpr (!PLAIN) asm volatile("" : "+s"(unext2));  // a scalar load's result, scalar till here
        unextv = unext2;
    }
#undef RCBF_OPAQUE_V
}

// Explicit instantiation of k_safe_steps for every mode / hazard count and
// workgroup size k_safe_step has (used once, by rcbf_env.hip): 27 kernels.
#define RCBF_SAFE_STEPS_INSTANTIATE_BS(MODE_, K_, BS_)                                                              \
    template __global__ void k_safe_steps<MODE_, K_, BS_>(                                                          \
        int64_t, double* __restrict__, double* __restrict__, int32_t* __restrict__, const float* const* __restrict__, \
        uint32_t* __restrict__, const float* __restrict__, const float* __restrict__, float* __restrict__,          \
        float* __restrict__, float* __restrict__, float* __restrict__, uint8_t* __restrict__, uint8_t* __restrict__, \
        int32_t* __restrict__, int32_t*, int, uint64_t, int64_t, rcbf_params, int, int, int, int)
#define RCBF_SAFE_STEPS_INSTANTIATE(MODE_, K_)      \
    RCBF_SAFE_STEPS_INSTANTIATE_BS(MODE_, K_, 64);  \
    RCBF_SAFE_STEPS_INSTANTIATE_BS(MODE_, K_, 128); \
    RCBF_SAFE_STEPS_INSTANTIATE_BS(MODE_, K_, 256)

}  // namespace rcbf
