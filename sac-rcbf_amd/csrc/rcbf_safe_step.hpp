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
// 1: k_safe_steps_traj stores the staged observation chunks as plain stores; 0 (the product): `nt`, as
// k_safe_steps does.  Nothing rewrites a recorded row, so `nt` is not the obvious choice there; measured
// (B = 65 536, all fields; profiles/r09/obs_store_flavour_traj_r09b.txt): `nt` 2.21 against plain 2.54 us per
// step at 20 cars steps and 3.21 / 3.31 (20), 2.49 / 2.53 (1 000) for the unicycle at k = 5, plain ahead only
// at 1 000 cars steps (1.90 against 1.95), five runs a side and the sets disjoint each time: `nt`.
#ifndef RCBF_TRAJ_OBS_PLAIN
#define RCBF_TRAJ_OBS_PLAIN 0
#endif
// 1: the cars step stores the state pairs that do not depend on the safe
// action before the layer's chain runs (k_safe_step; 3.86 -> 3.67 us per
// step, profiles/r03/early_store_confirm_r03k.txt); 0: after it
#ifndef RCBF_EARLY_STORE
#define RCBF_EARLY_STORE 1
#endif
// What the cars fused loop (k_safe_steps, k_safe_steps_traj) carries from a step's tail into the next step:
// 0: nothing, every step derives its layer's state from xs again (the per-step kernel's statements);
// 1 (the product): the fp32 observation row the tail has just computed for its store, which is the row the
//    next step's layer would compute again from the same xs;
// 2 (study): that row, and the next step's raw rows, built from it in the tail behind the LDS writes of the
//    observation staging instead of at the head of the next step's chain.  Slower than 1 in every leg of the
//    A/B (profiles/r10/ab_carry_vs_parent_r10a.txt): at the head the rows' arithmetic runs between the env's
//    pre-step fp64 chain, in the tail it only lengthens a stretch that has independent work already.
#ifndef RCBF_FUSED_CARRY
#define RCBF_FUSED_CARRY 1
#endif
// With the rows carried (RCBF_FUSED_CARRY == 2) the head of a step has nothing to build before it can solve.
// 0: the env's pre-step part and the early stores first, then the solve, as in the per-step kernel; 1: the
// solve first (the faster of the two with carried rows, same file; neither reaches RCBF_FUSED_CARRY == 1).
#ifndef RCBF_FUSED_CARRY_SOLVE_FIRST
#define RCBF_FUSED_CARRY_SOLVE_FIRST 0
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
// previous store.  SC1: the chunks leave write-through (st_out4); PLAIN_ST (gptr only): as plain stores.
template <int MODE, bool WT = false, bool SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS, typename OP = float*,
          bool PLAIN_ST = false, bool WHOLE = false>
__device__ __forceinline__ void store_obs_chunks(OP obs, int64_t base, const float* lds_wave, int lane) {
    constexpr int NO = Dims<MODE, 1>::NO;
    __builtin_amdgcn_wave_barrier();
    constexpr int CH = NO * 16;  // 16-byte chunks in the wave's block
    const float4* src = reinterpret_cast<const float4*>(lds_wave);
    const OP dst = obs + base * NO;
    constexpr int NJ = (CH + 63) / 64;
    float4 chunk[NJ];
    if constexpr (WHOLE) {
        // The cars fused loop's form: the first CH / 64 chunks are whole in the source, and the remainder
        // chunk's LDS read is unconditional too (a lane past the block reads its own first chunk again and
        // stores nothing), so that one lane test stands around one store and the reads share one wait.
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = j * 64 + lane;
            chunk[j] = src[(j < CH / 64 || c < CH) ? c : lane];
        }
        // every read is issued before the first store (nothing is emitted: the compiler otherwise moves the
        // remainder chunk's read, and a wait of its own, in behind the lane test)
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(chunk[j].x), "+v"(chunk[j].y), "+v"(chunk[j].z), "+v"(chunk[j].w));
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = j * 64 + lane;
            if (j < CH / 64 || c < CH) {
                if constexpr (PLAIN_ST)
                    st_out4_plain(dst + 4 * c, chunk[j]);
                else
                    st_out4<SC1>(dst + 4 * c, chunk[j]);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        if (CH % 64 == 0 || c < CH) chunk[j] = src[c];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = j * 64 + lane;
        if (CH % 64 == 0 || c < CH) {
            if constexpr (PLAIN_ST)
                st_out4_plain(dst + 4 * c, chunk[j]);
            else
                st_out4<SC1>(dst + 4 * c, chunk[j]);
        }
    }
}

// Observation store through LDS: a full wave's 64 obs rows are one
// contiguous (64*NO*4)-byte block; lanes write their rows into LDS, then
// store the block as 16-byte chunks, chunk c by lane c%64 -- every store
// instruction covers whole contiguous lines (cars: 3 dwordx4 instead of 5
// strided dwordx2).  Partial or unaligned waves take the per-lane path.
template <int MODE, bool WT = false, bool SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS, typename OP = float*,
          bool PLAIN_ST = false>
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
    store_obs_chunks<MODE, WT, SC1, OP, PLAIN_ST>(obs, base, lds_wave, lane);
}

// The first half of store_obs32_staged for a caller that already holds the fp32 observation row (the cars
// fused loop, which carries it into the next step): a full wave writes its 64 rows to LDS and returns true
// -- the caller calls store_obs_chunks later, after whatever it has to issue behind the LDS writes -- a
// partial or unaligned wave stores its row per lane, as store_obs32 does, and returns false.
template <int MODE, typename OP>
__device__ __forceinline__ bool stage_obs32_row(OP obs, int64_t i, int64_t B, const float* o32, float* lds_wave,
                                                int lane) {
    constexpr int NO = Dims<MODE, 1>::NO;
    static_assert(NO % 2 == 0, "8-byte halves of a row");
    const int64_t base = i - lane;
#ifdef RCBF_STUDY_EPW
    const bool full_l = blockDim.x != 64 && (base + 64 <= B) && ((reinterpret_cast<uintptr_t>(obs) & 15) == 0);
#else
    const bool full_l = (base + 64 <= B) && ((reinterpret_cast<uintptr_t>(obs) & 15) == 0);
#endif
    // the same in every lane of the wave (base is the wave's first env), which the compiler cannot see: read
    // from the first live lane it is a scalar, and the two paths a scalar branch instead of two lane masks
    const bool full = __builtin_amdgcn_readfirstlane((int)full_l) != 0;
    if (full) {
#pragma unroll
        for (int k = 0; k < NO / 2; ++k)
            *reinterpret_cast<float2*>(&lds_wave[lane * NO + 2 * k]) = make_float2(o32[2 * k], o32[2 * k + 1]);
    } else {
        const OP ov = obs + i * NO;  // 40 B rows, 8 B aligned
#pragma unroll
        for (int k = 0; k < NO / 2; ++k) st_out2(ov + 2 * k, o32[2 * k], o32[2 * k + 1]);
    }
    return full;
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
// chunks' store flavour (st_out4); OBS_PLAIN: plain stores instead (k_safe_steps_traj's study switch).
// TERM (k_safe_steps_term): a step that resets its env also stores, at term_obs[i], the observation of the
// post-step state BEFORE the reset -- the row this step would have stored with auto_reset = 0, bit for bit (the
// same env_obs / uni_obs_cs arithmetic and fp64 -> fp32 conversion) -- as per-lane `nt` dword stores; a step
// that does not reset writes nothing there.  Everything else a step computes and stores is as with TERM off,
// and with TERM off every statement about it is discarded.
template <int SOLVER, int MODE, int K, bool ST, bool WT, bool GP = false,
          bool OBS_SC1 = WT || MODE == RCBF_MODE_SIMULATED_CARS, bool OBS_PLAIN = false, int CARRY = 0,
          bool TERM = false>
__device__ __forceinline__ void safe_step_body(
    const rcbf_params& prm, int64_t B, int64_t i, ptr_g<GP, double> __restrict__ x, ptr_g<GP, double> __restrict__ aux,
    ptr_g<GP, int32_t> __restrict__ step, ptr_g<GP, uint32_t> __restrict__ episode,
    ptr_g<GP, float> __restrict__ obs_out, ptr_g<GP, float> __restrict__ u_out, ptr_g<GP, float> __restrict__ reward,
    ptr_g<GP, float> __restrict__ cost, ptr_g<GP, uint8_t> __restrict__ done, ptr_g<GP, uint8_t> __restrict__ goal_met,
    ptr_g<GP, int32_t> __restrict__ status_out, ptr_g<GP, int32_t> fail_flag, int auto_reset,
    uint64_t seed, int64_t off, double* xs, double& a, int& st, const float* us, const float* m, const float* s,
    bool ep_pre, uint32_t ep0, const Stamps<ST>& stamps, float* obs_stage, char* wt_lds, int lane,
    bool* did_reset = nullptr, float* obs_c = nullptr, float (*G_c)[Dims<MODE, K>::N] = nullptr,
    float* h_c = nullptr, const float* u_nx = nullptr, ptr_g<GP, float> term_obs = nullptr) {
    using D = Dims<MODE, K>;
    static_assert(!TERM || (GP && !ST && !WT && SOLVER == RCBF_SOLVER_ACTIVE_SET &&
                            (MODE != RCBF_MODE_SIMULATED_CARS || RCBF_EARLY_STORE)),
                  "the terminal observation: the fused loop only");
    static_assert(CARRY == 0 || (MODE == RCBF_MODE_SIMULATED_CARS && RCBF_EARLY_STORE && !ST && !WT && GP &&
                                 SOLVER == RCBF_SOLVER_ACTIVE_SET && RCBF_FUSED_RAW_ROWS != 0),
                  "the carried observation: the cars fused loop only");
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
        if constexpr (CARRY == 0) state_from_env<MODE>(xs, s32);  // the layer reads the pre-step state
        if constexpr (CARRY == 1) state_from_obs32<MODE>(obs_c, s32);  // ... through the row the last step stored
        // the exact solver on the raw rows: the rows are built here, ahead of
        // the env's pre-step part, whose arithmetic can then fill their latency
        // (3.69 -> 3.65 us per step, profiles/r03/rows_first_ab_r03q.txt)
        constexpr bool kRowsFirst = SOLVER == RCBF_SOLVER_ACTIVE_SET && RCBF_FUSED_RAW_ROWS != 0;
        LayerState<MODE, K> L;
        if constexpr (CARRY == 2) {
            // ... and the rows themselves were built in the last step's tail
#pragma unroll
            for (int r = 0; r < D::M; ++r) {
                L.h[r] = h_c[r];
#pragma unroll
                for (int k = 0; k < D::N; ++k) L.G[r][k] = G_c[r][k];
            }
        } else if constexpr (kRowsFirst) {
            diff_rows<MODE, K>(prm, s32, us, m, s, L.G, L.h, nullptr);
        }
        constexpr bool kSolveFirst = CARRY == 2 && RCBF_FUSED_CARRY_SOLVE_FIRST != 0;
        if constexpr (kSolveFirst) {
            layer_solve_raw<MODE, K>(prm, us, uf, L);
            __builtin_amdgcn_sched_barrier(0);
        }
        CarsStepOut o;
        const double acc3 = cars_env_pre(prm, xs, a, st, o);
        dn = o.done;
        cst = (float)o.cost;
        gm = false;
        const bool rs = auto_reset && dn;
        if (rs) {
            if constexpr (TERM) {
                // the terminal row but for car 3's velocity (component 7), which follows the solve
                double ot[D::NO];
                env_obs<MODE>(xs, ot);
#pragma unroll
                for (int k = 0; k < D::NO; ++k)
                    if (k != 7) st_out(&term_obs[i * D::NO + k], (float)ot[k]);
                oc[0] = xs[7];  // car 3's velocity before the reset, which the action below completes (oc is
                                // otherwise the unicycle's: nothing else on this path reads it)
            }
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
        if constexpr (kSolveFirst) {
            // solved above
        } else if constexpr (kRowsFirst) {
            layer_solve_raw<MODE, K>(prm, us, uf, L);  // the same solve as layer_forward<..., RAW>
        } else {
            layer_forward<SOLVER, MODE, K, false, false, RCBF_FUSED_RAW_ROWS != 0>(prm, s32, us, m, s, uf, L);
        }
        status = L.qp.status;
        const double v3_reset = xs[7];
        if constexpr (TERM) xs[7] = rs ? oc[0] : xs[7];  // a resetting lane finishes the velocity it had
        cars_env_post<float>(xs, acc3, uf[0], o);  // car 3's velocity and the reward
        if constexpr (TERM) {
            if (rs) st_out(&term_obs[i * D::NO + 7], (float)div_const(xs[7], 30.0, 1.0 / 30.0));  // cars_obs
        }
        xs[7] = rs ? v3_reset : xs[7];
        rew = o.reward;
        st_any2d<WT>(&x[2 * (3 * B + i)], xs[6], xs[7]);
    } else {
        if constexpr (TERM) {
            static_assert(MODE == RCBF_MODE_UNICYCLE, "the cars loop takes the early-store path");
            // the step without its reset (oc: cos, sin and goal distance of the post-step state) ...
            safe_step_one<SOLVER, MODE, K, ST, WT>(prm, i, xs, a, st, episode, us, m, s, uf, rew, cst, dn, gm, status,
                                                   0, seed, off, stamps, oc, ep_pre, ep0);
            if (auto_reset && dn) {
                // ... the row store_obs32 would store of it, then the reset, in safe_step_one's statements
                double ot[D::NO];
                uni_obs_cs(xs, oc[0], oc[1], oc[2], ot);
#pragma unroll
                for (int k = 0; k < D::NO; ++k) st_out(&term_obs[i * D::NO + k], (float)ot[k]);
                const uint32_t ep = episode ? (ep_pre ? ep0 : episode[i]) + 1u : 0u;
                if (episode) episode[i] = ep;
                env_reset_one<MODE>(nullptr, i, seed, off, ep, xs, a, st);
                oc[0] = 1.0;  // the reset state's obs inputs
                oc[1] = 0.0;
                oc[2] = a;
                oc[3] = 1.0;
            }
        } else {
            safe_step_one<SOLVER, MODE, K, ST, WT>(prm, i, xs, a, st, episode, us, m, s, uf, rew, cst, dn, gm, status,
                                                   auto_reset, seed, off, stamps, oc, ep_pre, ep0);
        }
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
    bool obs_staged = false;
    if constexpr (CARRY != 0) {
        // The observation of the post-step (or reset) state, computed once: the row stored here is the row the
        // next step's layer reads (obs_c).  A full wave's rows go to LDS now and leave as chunks at the end of
        // the step; behind the LDS writes come the next step's state32 and rows (CARRY == 2: from obs_c, the
        // priors and the next action, all in registers) and this step's u, reward, cost and done stores.
        double o[D::NO];
        env_obs<MODE>(xs, o);
#pragma unroll
        for (int k = 0; k < D::NO; ++k) obs_c[k] = (float)o[k];
        obs_staged = stage_obs32_row<MODE>(obs_out, i, B, obs_c, obs_stage, lane);
        if constexpr (CARRY == 2) {
            float s32n[D::NS];
            state_from_obs32<MODE>(obs_c, s32n);
            diff_rows<MODE, K>(prm, s32n, u_nx, m, s, G_c, h_c, nullptr);
            // the rows are finished here, behind the LDS writes and ahead of the stores below (nothing is emitted;
            // the compiler otherwise moves their arithmetic behind the chunk stores, to where the next step
            // reads them); the other entries of G are constants
            asm volatile("" : "+v"(G_c[0][0]), "+v"(G_c[1][0]), "+v"(h_c[0]), "+v"(h_c[1]), "+v"(h_c[2]), "+v"(h_c[3]));
        }
    } else {
        store_obs32_staged<MODE, WT, OBS_SC1, ptr_g<GP, float>, OBS_PLAIN>(obs_out, i, B, xs, oc, obs_stage, lane);
    }
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
    if constexpr (CARRY != 0) {
        if (obs_staged)
            store_obs_chunks<MODE, WT, OBS_SC1, ptr_g<GP, float>, OBS_PLAIN, true>(obs_out, wbase, obs_stage, lane);
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
// TRAJ (k_safe_steps_traj): no kernel is plain.  With the recorded outputs' pointers changing every step the
// cars kernel and the unicycle at k = 1, written plain, spill 5 and 2 scalar registers (64-thread workgroups).
template <int MODE>
constexpr int fused_carry() {
    return MODE == RCBF_MODE_SIMULATED_CARS ? RCBF_FUSED_CARRY : 0;
}

template <int MODE, int K, bool TRAJ = false>
constexpr bool fused_plain() {
    return !TRAJ && (MODE == RCBF_MODE_SIMULATED_CARS || K == 1);
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
//
// k_safe_steps_traj (the trajectory form, rcbf_aql_safe_step_traj_plan): the same loop, which after every
// step moves each RECORDED output's pointer on by one row of its dense (steps, P, w) array, P = traj_pitch
// envs, w the output's per-env width: step j's values stay at [j][i] instead of being overwritten by step
// j + 1.  traj_mask (RCBF_TRAJ_*, rcbf_hip.h) says which outputs are recorded; the others, and x, aux, step,
// episode, fail_flag always, are written in place as in k_safe_steps.  The builder clears the bit of a null
// pointer (a null pointer moved on is no longer null to the step's `if (goal_met)`), and checks P >= B,
// P % 4 == 0 and a 16-byte aligned recorded obs base, which keep every 16-byte observation chunk aligned in
// every row (store_obs_chunks).  Its argument block is SafeStepsArgs followed by traj_mask and traj_pitch:
struct SafeStepsTrajArgs {
    SafeStepsArgs s;
    int32_t traj_mask;
    int64_t traj_pitch;
};
static_assert(offsetof(SafeStepsTrajArgs, traj_mask) == 408 && offsetof(SafeStepsTrajArgs, traj_pitch) == 416 &&
                  sizeof(SafeStepsTrajArgs) == 424,
              "kernarg layout");

// traj_mask and traj_pitch as the loop carries them (k = 8: this wave's copy in LDS)
struct TrajTail {
    int64_t pitch;
    int32_t mask;
    int32_t pad;
};

// ... read from k_safe_steps_traj's argument segment, `off` (0, or a zero the compiler cannot see through)
// bytes on: uniform loads from the constant address space, so scalar loads wherever they stand
__device__ __forceinline__ TrajTail traj_from_kernargs(uint32_t off) {
    TrajTail t{0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const char __attribute__((address_space(4)))* cbytes_t;
    const cbytes_t ka = (cbytes_t)__builtin_amdgcn_kernarg_segment_ptr() + off;
    t.mask = *reinterpret_cast<const int32_t __attribute__((address_space(4)))*>(
        ka + offsetof(SafeStepsTrajArgs, traj_mask));
    t.pitch = *reinterpret_cast<const int64_t __attribute__((address_space(4)))*>(
        ka + offsetof(SafeStepsTrajArgs, traj_pitch));
#endif
    return t;
}

template <int BS>
__device__ __forceinline__ TrajTail* traj_stage_of(int wave) {
    __shared__ TrajTail stage[BS / 64];
    return &stage[wave];
}

// The trajectory form that also keeps the terminal observation (rcbf_aql_safe_step_term_plan, traj_mask with
// RCBF_TRAJ_TERM_OBS): k_safe_steps_traj with one more recorded pointer, term_obs, the base of a dense
// (steps, P, n_o) fp32 array.  A step j that resets env i stores at [j][i] the observation of env i's post-step
// state before the reset (safe_step_body, TERM); nothing else of the array is written.  The pointer is moved on
// by one row per step like the other recorded pointers.  Its argument block is SafeStepsTrajArgs + term_obs:
struct SafeStepsTermArgs {
    SafeStepsTrajArgs t;
    float* term_obs;
};
static_assert(offsetof(SafeStepsTermArgs, term_obs) == 424 && sizeof(SafeStepsTermArgs) == 432, "kernarg layout");

// ... read from the argument segment like traj_mask and traj_pitch (the loop's source names no parameter that
// only one of the three kernels has)
__device__ __forceinline__ gptr<float> term_from_kernargs() {
    uint64_t p = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const char __attribute__((address_space(4)))* cbytes_t;
    const cbytes_t ka = (cbytes_t)__builtin_amdgcn_kernarg_segment_ptr();
    p = *reinterpret_cast<const uint64_t __attribute__((address_space(4)))*>(
        ka + offsetof(SafeStepsTermArgs, term_obs));
#endif
    return reinterpret_cast<gptr<float>>(p);
}

// The loop's source is one file, rcbf_safe_steps_loop.inc, included as the body of both kernels: with TRAJ =
// false every `if constexpr (TRAJ)` in it is discarded and k_safe_steps is, statement for statement, the
// kernel it was before the trajectory form existed (and compiles to the same machine code, which a common
// device function inlined into it did not: the inlined copy came out with other branches and registers).
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
    constexpr bool TRAJ = false;
#define RCBF_LOOP_TERM 0
#include "rcbf_safe_steps_loop.inc"
#undef RCBF_LOOP_TERM
}

// The trajectory form (SafeStepsTrajArgs above).  traj_mask and traj_pitch are part of the argument block and
// read from it by the loop where it uses them, not through these two parameters.
template <int MODE, int K, int BS = kBlock>
__global__ void __launch_bounds__(BS) k_safe_steps_traj(
    int64_t B, double* __restrict__ x, double* __restrict__ aux, int32_t* __restrict__ step,
    const float* const* __restrict__ u_tab, uint32_t* __restrict__ episode, const float* __restrict__ mu,
    const float* __restrict__ sigma, float* __restrict__ obs_out, float* __restrict__ u_out,
    float* __restrict__ reward, float* __restrict__ cost, uint8_t* __restrict__ done, uint8_t* __restrict__ goal_met,
    int32_t* __restrict__ status_out, int32_t* fail_flag, int auto_reset, uint64_t seed, int64_t off, rcbf_params prm,
    int prior_cols, int n_u, int steps, int ju0, int32_t traj_mask, int64_t traj_pitch) {
    (void)traj_mask;
    (void)traj_pitch;
    constexpr bool TRAJ = true;
#define RCBF_LOOP_TERM 0
#include "rcbf_safe_steps_loop.inc"
#undef RCBF_LOOP_TERM
}

// The trajectory form that also keeps the terminal observation (SafeStepsTermArgs above).
template <int MODE, int K, int BS = kBlock>
__global__ void __launch_bounds__(BS) k_safe_steps_term(
    int64_t B, double* __restrict__ x, double* __restrict__ aux, int32_t* __restrict__ step,
    const float* const* __restrict__ u_tab, uint32_t* __restrict__ episode, const float* __restrict__ mu,
    const float* __restrict__ sigma, float* __restrict__ obs_out, float* __restrict__ u_out,
    float* __restrict__ reward, float* __restrict__ cost, uint8_t* __restrict__ done, uint8_t* __restrict__ goal_met,
    int32_t* __restrict__ status_out, int32_t* fail_flag, int auto_reset, uint64_t seed, int64_t off, rcbf_params prm,
    int prior_cols, int n_u, int steps, int ju0, int32_t traj_mask, int64_t traj_pitch, float* __restrict__ term_obs) {
    (void)traj_mask;
    (void)traj_pitch;
    (void)term_obs;
    constexpr bool TRAJ = true;
#define RCBF_LOOP_TERM 1
#include "rcbf_safe_steps_loop.inc"
#undef RCBF_LOOP_TERM
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

// ... and of k_safe_steps_traj: the same 27
#define RCBF_SAFE_STEPS_TRAJ_INSTANTIATE_BS(MODE_, K_, BS_)                                                         \
    template __global__ void k_safe_steps_traj<MODE_, K_, BS_>(                                                     \
        int64_t, double* __restrict__, double* __restrict__, int32_t* __restrict__, const float* const* __restrict__, \
        uint32_t* __restrict__, const float* __restrict__, const float* __restrict__, float* __restrict__,          \
        float* __restrict__, float* __restrict__, float* __restrict__, uint8_t* __restrict__, uint8_t* __restrict__, \
        int32_t* __restrict__, int32_t*, int, uint64_t, int64_t, rcbf_params, int, int, int, int, int32_t, int64_t)
#define RCBF_SAFE_STEPS_TRAJ_INSTANTIATE(MODE_, K_)      \
    RCBF_SAFE_STEPS_TRAJ_INSTANTIATE_BS(MODE_, K_, 64);  \
    RCBF_SAFE_STEPS_TRAJ_INSTANTIATE_BS(MODE_, K_, 128); \
    RCBF_SAFE_STEPS_TRAJ_INSTANTIATE_BS(MODE_, K_, 256)

// ... and of k_safe_steps_term (rcbf_steps_term.hip): the same 27
#define RCBF_SAFE_STEPS_TERM_INSTANTIATE_BS(MODE_, K_, BS_)                                                         \
    template __global__ void k_safe_steps_term<MODE_, K_, BS_>(                                                     \
        int64_t, double* __restrict__, double* __restrict__, int32_t* __restrict__, const float* const* __restrict__, \
        uint32_t* __restrict__, const float* __restrict__, const float* __restrict__, float* __restrict__,          \
        float* __restrict__, float* __restrict__, float* __restrict__, uint8_t* __restrict__, uint8_t* __restrict__, \
        int32_t* __restrict__, int32_t*, int, uint64_t, int64_t, rcbf_params, int, int, int, int, int32_t, int64_t, \
        float* __restrict__)
#define RCBF_SAFE_STEPS_TERM_INSTANTIATE(MODE_, K_)      \
    RCBF_SAFE_STEPS_TERM_INSTANTIATE_BS(MODE_, K_, 64);  \
    RCBF_SAFE_STEPS_TERM_INSTANTIATE_BS(MODE_, K_, 128); \
    RCBF_SAFE_STEPS_TERM_INSTANTIATE_BS(MODE_, K_, 256)

}  // namespace rcbf
