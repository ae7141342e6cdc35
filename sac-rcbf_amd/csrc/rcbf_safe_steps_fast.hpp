// rcbf_safe_steps_fast.hpp -- rcbf::k_safe_steps_fast, the cars fused plan's loop laid out for the instruction
// scheduler (rcbf_steps_fast.hip instantiates it; librcbf_steps_fast.co).  It computes and stores, step for step
// and bit for bit, what rcbf::k_safe_steps<RCBF_MODE_SIMULATED_CARS, 1, BS> does, from the same argument block
// (SafeStepsArgs), and the plan builder (csrc/rcbf_aql.hip) dispatches it in that kernel's place when
//   - every wave is full (B % 64 == 0) and the observation buffer is 16-byte aligned, so every wave stages its
//     rows through LDS and no per-lane observation path exists;
//   - goal_met and status_out are null, episode and fail_flag are not (what BatchedEnv._step_args passes for cars).
// One wave per SIMD runs this loop (65 536 envs are 1 024 waves), so what a step costs is what one wave can
// issue, and the loop is written so that the scheduler sees long regions:
//   - the tests that cannot change during a plan are resolved by the builder (above): the step has none;
//   - the lead car's sine is sin_small's series for every lane (cars_env_pre<true>).  Before each iteration a
//     ballot asks whether |0.2 t| <= 1.3 holds in every lane for the steps of the iteration; when it does not,
//     the wave leaves this loop for good and runs its remaining steps through safe_step_body, exactly as
//     k_safe_steps does (the second loop below): lanes in range get the series' bits there too;
//   - the reset stays per lane with its arithmetic and draw, but reads seed and off from the argument segment
//     inside its block, so the Philox keys are not held in scalar registers across the step;
//   - the reward's division by 300 is div_f32_via_rcp (cars_env_post<float, true>);
//   - the failed-solve bits of an iteration's steps are ORed into fail_flag once, at the iteration's end;
//   - RCBF_FAST_PAIR (the product): an iteration is two steps, in the order head A, mid A, head B, chunks A,
//     mid B, chunks B (cars_fast_head / _mid / _chunks below), so the second step's rows, sine and cars 0, 1, 2, 4
//     stand between the first step's LDS writes and its chunk reads, and no branch between the two steps: the
//     last half round of observation chunks is stored without a lane test (store_obs_chunks_full).  Both actions
//     of the next iteration are loaded at an iteration's head, through table entries fetched the iteration
//     before, and taken over at its end; every entry of the table is a buffer of B actions, so the loads need no
//     test of the step count.  A plan's odd last step runs in the second loop;
//   - without RCBF_FAST_PAIR (study): one step per iteration, which loads the action of step j + 2
//     (RCBF_FAST_AHEAD2) or j + 1 during step j.
// Every store of every step is made in that step, with k_safe_steps's flavours and the LDS-staged 16-byte
// observation chunks, and the compiler barrier between two steps keeps it so.
// Measured (profiles/r16/ab_fast_vs_parent_r16a.txt; B = 65 536, us per step at 20 / 1 000 steps, five process
// medians a side): k_safe_steps 1.72-1.84 / 1.31-1.41; one step per iteration, one ahead 1.64-1.74 / 1.20-1.33;
// two ahead 1.64-1.78 / 1.25-1.42 (no gain by itself: not kept in that form); the pair form 1.50-1.64 / 1.11-1.21.
#pragma once

#include "rcbf_safe_step.hpp"

// study switches (profiles/README.md): the product is both on; RCBF_FAST_PAIR=0 alone and with RCBF_FAST_AHEAD2=0
// are the one-step forms measured on the way
#ifndef RCBF_FAST_PAIR
#define RCBF_FAST_PAIR 1
#endif
#ifndef RCBF_FAST_AHEAD2
#define RCBF_FAST_AHEAD2 1
#endif

namespace rcbf {

// seed and off of the argument block, read `koff` (a zero the compiler cannot see through) bytes on: scalar loads
// that stay where they are asked for (the reset's block)
__device__ __forceinline__ void seed_off_from_kernargs(uint32_t koff, uint64_t& seed, int64_t& off) {
    seed = 0;
    off = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const char __attribute__((address_space(4)))* cbytes_t;
    const cbytes_t ka = (cbytes_t)__builtin_amdgcn_kernarg_segment_ptr() + koff;
    seed = *reinterpret_cast<const uint64_t __attribute__((address_space(4)))*>(ka + offsetof(SafeStepsArgs, seed));
    off = *reinterpret_cast<const int64_t __attribute__((address_space(4)))*>(ka + offsetof(SafeStepsArgs, off));
#endif
}

// store_obs_chunks for a full wave of cars rows without a lane test: the block is 160 16-byte chunks, two whole
// rounds of 64 and a last round of 32.  In the last round lane l and lane l + 32 both store chunk 128 + l % 32, the
// same bytes to the same address in one instruction, so no branch stands between this step's tail and the next
// step's head and the bytes that reach memory are store_obs_chunks's.  `nt`, as the fused loop's chunks are.
__device__ __forceinline__ void store_obs_chunks_full(gptr<float> obs, int64_t base, const float* lds_wave, int lane) {
    constexpr int NO = Dims<RCBF_MODE_SIMULATED_CARS, 1>::NO;
    static_assert(NO * 16 == 2 * 64 + 32, "two whole rounds and half a round of chunks");
    __builtin_amdgcn_wave_barrier();
    const float4* src = reinterpret_cast<const float4*>(lds_wave);
    const gptr<float> dst = obs + base * NO;
    const int c2 = 128 + (lane & 31);
    const float4 k0 = src[lane], k1 = src[64 + lane], k2 = src[c2];
    st_out4<false>(dst + 4 * lane, k0);
    st_out4<false>(dst + 4 * (64 + lane), k1);
    st_out4<false>(dst + 4 * c2, k2);
}

// One step of env i on a full wave is safe_step_body's cars early-store order with the carried observation row
// (CARRY == 1), without its tests, in three parts, so that the pair form can set the next step's head between a
// step's LDS writes and its chunk reads:
//   cars_fast_head    what needs neither the safe action nor memory: the layer's rows from the carried row, the
//                     env's pre-step part (series sine), done, cost;
//   cars_fast_mid     the reset (rare, per lane), the early stores, the solve, car 3's velocity and the reward, the
//                     new observation row to LDS, the u, reward, cost and done stores;
//   cars_fast_chunks  the observation block's chunks from LDS to memory, and the barrier that ends a step's stores.
struct CarsFastHead {
    LayerState<RCBF_MODE_SIMULATED_CARS, 1> L;
    double acc3;
    float u_rl, cst;
    bool dn;
};

__device__ __forceinline__ void cars_fast_head(const rcbf_params& prm, double* xs, double& a, int& st, float u_rl,
                                               const float* m, const float* s, const float* obs_c, CarsFastHead& h) {
    constexpr int MODE = RCBF_MODE_SIMULATED_CARS;
    using D = Dims<MODE, 1>;
    const float us[1] = {u_rl};
    float s32[D::NS];
    state_from_obs32<MODE>(obs_c, s32);  // the layer reads the pre-step state through the row the last step stored
    diff_rows<MODE, 1>(prm, s32, us, m, s, h.L.G, h.L.h, nullptr);
    CarsStepOut o;
    h.acc3 = cars_env_pre<true>(prm, xs, a, st, o);
    h.dn = o.done;
    h.cst = (float)o.cost;
    h.u_rl = u_rl;
}

// fail_bits collects 1 << status of a failed solve
__device__ __forceinline__ void cars_fast_mid(const rcbf_params& prm, int64_t B, int64_t i, gptr<double> x,
                                              gptr<double> aux, gptr<int32_t> step, gptr<uint32_t> episode,
                                              gptr<float> u_out, gptr<float> reward, gptr<float> cost,
                                              gptr<uint8_t> done, int auto_reset, double* xs, double& a, int& st,
                                              uint32_t& epr, float* obs_c, float* obs_stage, int lane, int& fail_bits,
                                              CarsFastHead& h) {
    constexpr int MODE = RCBF_MODE_SIMULATED_CARS;
    using D = Dims<MODE, 1>;
    const bool rs = auto_reset && h.dn;
    if (__builtin_expect(rs, 0)) {
        uint32_t koff = 0;
        asm volatile("" : "+s"(koff));
        uint64_t seed;
        int64_t off;
        seed_off_from_kernargs(koff, seed, off);
        const uint32_t ep = epr + 1u;
        episode[i] = ep;
        epr = ep;
        env_reset_one<MODE>(nullptr, i, seed, off, ep, xs, a, st);
    }
#pragma unroll
    for (int p = 0; p < D::NS / 2; ++p)
        if (p != 3) st_out2d(&x[2 * (p * B + i)], xs[2 * p], xs[2 * p + 1]);
    st_out(&aux[i], a);
    st_out(&step[i], st);
    __builtin_amdgcn_sched_barrier(0);  // keep the early stores ahead of the layer's chain
    const float us[1] = {h.u_rl};
    float uf[1];
    layer_solve_raw<MODE, 1>(prm, us, uf, h.L);
    const int status = h.L.qp.status;
    const double v3_reset = xs[7];
    CarsStepOut o;
    cars_env_post<float, true>(xs, h.acc3, uf[0], o);  // car 3's velocity and the reward
    xs[7] = rs ? v3_reset : xs[7];
    st_out2d(&x[2 * (3 * B + i)], xs[6], xs[7]);
    // the observation of the post-step (or reset) state: the row stored here is the row the next step's layer reads
    double ob[D::NO];
    env_obs<MODE>(xs, ob);
#pragma unroll
    for (int k = 0; k < D::NO; ++k) obs_c[k] = (float)ob[k];
#pragma unroll
    for (int k = 0; k < D::NO / 2; ++k)
        *reinterpret_cast<float2*>(&obs_stage[lane * D::NO + 2 * k]) = make_float2(obs_c[2 * k], obs_c[2 * k + 1]);
    st_out(&u_out[i], uf[0]);
    st_out(&reward[i], o.reward);
    st_out(&cost[i], h.cst);
    st_out(&done[i], (uint8_t)h.dn);
    fail_bits |= status != RCBF_QP_OK ? 1 << status : 0;
}

__device__ __forceinline__ void cars_fast_chunks(int64_t i, gptr<double> x, gptr<double> aux, gptr<int32_t> step,
                                                 gptr<float> obs_out, gptr<float> u_out, gptr<float> reward,
                                                 gptr<float> cost, gptr<uint8_t> done, float* obs_stage, int lane) {
    if constexpr (RCBF_FAST_PAIR != 0)
        store_obs_chunks_full(obs_out, i - lane, obs_stage, lane);
    else
        store_obs_chunks<RCBF_MODE_SIMULATED_CARS, false, false, gptr<float>, false, true>(obs_out, i - lane,
                                                                                           obs_stage, lane);
    // this step's chunk reads of obs_stage stay ahead of the next step's writes to it
    __builtin_amdgcn_wave_barrier();
    // every step's stores are made in that step (rcbf_safe_steps_loop.inc).  The buffers' bases go in as operands
    // (scalar registers they are in anyway): two steps stand in one block here, and without the observation's the
    // first step's whole chunks, which the second step's overwrite, were dropped (each buffer is a `noalias`
    // argument that otherwise never escapes).
    asm volatile("" ::"s"(obs_out), "s"(x), "s"(aux), "s"(step), "s"(u_out), "s"(reward), "s"(cost), "s"(done) : "memory");
}

template <int BS = kBlock>
__global__ void __launch_bounds__(BS) k_safe_steps_fast(
    int64_t B, double* __restrict__ x, double* __restrict__ aux, int32_t* __restrict__ step,
    const float* const* __restrict__ u_tab, uint32_t* __restrict__ episode, const float* __restrict__ mu,
    const float* __restrict__ sigma, float* __restrict__ obs_out, float* __restrict__ u_out,
    float* __restrict__ reward, float* __restrict__ cost, uint8_t* __restrict__ done, uint8_t* __restrict__ goal_met,
    int32_t* __restrict__ status_out, int32_t* fail_flag, int auto_reset, uint64_t seed, int64_t off, rcbf_params prm,
    int prior_cols, int n_u, int steps, int ju0) {
    constexpr int MODE = RCBF_MODE_SIMULATED_CARS;
    using D = Dims<MODE, 1>;
    static_assert(D::NU == 1 && RCBF_EARLY_STORE && RCBF_FUSED_RAW_ROWS != 0, "the cars fused step's product form");
    (void)goal_met;    // null, by the builder's condition
    (void)status_out;  // likewise
    const int64_t i = env_index<BS>();
    if (i >= B) return;  // never: B % 64 == 0 and the grid is ceil(B / BS) workgroups
    double xs[D::NS];
    load_state<MODE>(x, B, i, xs);
    double a = ld_in(&aux[i]);
    int st = ld_in(&step[i]);
    // the u_RL table, read with scalar loads (rcbf_safe_steps_loop.inc)
    typedef const uint64_t __attribute__((address_space(4)))* ctab_t;
    const ctab_t tab = (ctab_t)reinterpret_cast<const uint64_t*>(u_tab);
    auto next_j = [n_u](int j) { return j + 1 == n_u ? 0 : j + 1; };
    // What both loops carry of the table's walk, at a step j's head.  u0: step j's action.  RCBF_FAST_AHEAD2: u1,
    // step j + 1's action, and p2, the buffer of step j + 2, whose load step j issues; RCBF_FAST_PAIR also p3, the
    // buffer of step j + 3 (an iteration asks for both actions of the next iteration at its head).  Without
    // RCBF_FAST_AHEAD2 (and RCBF_FAST_PAIR): p2 is step j + 1's buffer.  ju: the table index of the last buffer held.
    static_assert(RCBF_FAST_AHEAD2 || !RCBF_FAST_PAIR, "the pair form loads two steps ahead");
    float u0 = ld_in(&reinterpret_cast<gptr<const float>>(tab[ju0])[i]);
    int ju = next_j(ju0);
    float u1 = 0.0f;
#if RCBF_FAST_AHEAD2
    u1 = ld_in(&reinterpret_cast<gptr<const float>>(tab[ju])[i]);
    ju = next_j(ju);
#endif
    uint64_t p2 = tab[ju], p3 = 0;
#if RCBF_FAST_PAIR
    ju = next_j(ju);
    p3 = tab[ju];
#endif
    uint32_t epr = ld_in(&episode[i]);
    prefetch_kernargs<7>();
    // the priors: inputs of the plan that nothing in a run writes, loaded once (k_safe_step's layouts)
    float m[D::NS], s[D::NS];
    if (prior_cols) {
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = 0.0f;
            s[k] = prior_sigma<MODE>(k);
        }
        if (sigma) {
            s[5] = ld_in(&sigma[i]);
            s[7] = ld_in(&sigma[B + i]);
            s[9] = ld_in(&sigma[2 * B + i]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < D::NS; ++k) {
            m[k] = mu ? mu[i * D::NS + k] : 0.0f;
            s[k] = sigma ? sigma[i * D::NS + k] : prior_sigma<MODE>(k);
        }
    }
    __shared__ float obs_stage[BS / 64][64 * D::NO];
    const gptr<double> xv = (gptr<double>)x;
    const gptr<double> auxv = (gptr<double>)aux;
    const gptr<int32_t> stepv = (gptr<int32_t>)step;
    gptr<uint32_t> epv = (gptr<uint32_t>)episode;
    const gptr<float> obsv = (gptr<float>)obs_out;
    const gptr<float> uv = (gptr<float>)u_out;
    const gptr<float> rewv = (gptr<float>)reward;
    const gptr<float> costv = (gptr<float>)cost;
    const gptr<uint8_t> donev = (gptr<uint8_t>)done;
    gptr<int32_t> failv = (gptr<int32_t>)fail_flag;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int left = steps;
    // everything loaded so far has arrived before a loop is entered (vmcnt(0); rcbf_safe_steps_loop.inc)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    float obs_c[D::NO];
    {
        double o[D::NO];
        env_obs<MODE>(xs, o);
#pragma unroll
        for (int k = 0; k < D::NO; ++k) obs_c[k] = (float)o[k];
    }
    // The walk, one step on: the head asks for the action two steps ahead (or one) and fetches the buffer address
    // behind the last one held (a scalar load, whether or not that step runs: every entry of the table is a buffer
    // of B actions); the tail moves the carried values up.
#define RCBF_FAST_WALK_HEAD()                                             \
    const float un_ = ld_in(&reinterpret_cast<gptr<const float>>(p2)[i]); \
    ju = next_j(ju);                                                      \
    const uint64_t pn_ = tab[ju]
#if RCBF_FAST_PAIR
#define RCBF_FAST_WALK_TAIL() \
    u0 = u1;                  \
    u1 = un_;                 \
    p2 = p3;                  \
    p3 = pn_
#elif RCBF_FAST_AHEAD2
#define RCBF_FAST_WALK_TAIL() \
    u0 = u1;                  \
    u1 = un_;                 \
    p2 = pn_
#else
#define RCBF_FAST_WALK_TAIL() \
    u0 = un_;                 \
    p2 = pn_
#endif
#define RCBF_FAST_MID(H_)                                                                                           \
    cars_fast_mid(prm, B, i, xv, auxv, stepv, epv, uv, rewv, costv, donev, auto_reset, xs, a, st, epr, obs_c, \
                  obs_stage[wid], lane, fail_bits, H_)
#define RCBF_FAST_CHUNKS() cars_fast_chunks(i, xv, auxv, stepv, obsv, uv, rewv, costv, donev, obs_stage[wid], lane)
    constexpr int PER = RCBF_FAST_PAIR ? 2 : 1;
#pragma nounroll
    while (left >= PER) {
        // |0.2 t| <= 1.3 in every lane at each step of this iteration (a step leaves t + 0.02, or 0 after a reset)?
        bool in_range = fabs(0.2 * a) <= 1.3;
        if (PER == 2) in_range = in_range && fabs(0.2 * (a + 0.02)) <= 1.3;
        if (__builtin_amdgcn_ballot_w64(!in_range) != 0) break;
        // the two pointers that only a reset and a failed solve use, as per-lane values (no instruction): their
        // addresses are worked out where those rare paths need them, not held in scalar registers over the step
        asm volatile("" : "+v"(epv), "+v"(failv));
        int fail_bits = 0;
        left -= PER;
#if RCBF_FAST_PAIR
        // both actions of the next iteration are asked for here and taken over at this iteration's end, two steps
        // later: nothing of the walk stands between the two steps, and the copies wait for no store of theirs
        const float n0 = ld_in(&reinterpret_cast<gptr<const float>>(p2)[i]);
        const float n1 = ld_in(&reinterpret_cast<gptr<const float>>(p3)[i]);
        ju = next_j(ju);
        const uint64_t q2 = tab[ju];
        ju = next_j(ju);
        const uint64_t q3 = tab[ju];
        CarsFastHead ha, hb;
        cars_fast_head(prm, xs, a, st, u0, m, s, obs_c, ha);
        RCBF_FAST_MID(ha);
        // the second step's head between the first step's LDS writes and its chunk reads (nothing is emitted for
        // the two barriers; left alone, the scheduler sets the reads and their wait right behind the writes)
        __builtin_amdgcn_sched_barrier(0);
        cars_fast_head(prm, xs, a, st, u1, m, s, obs_c, hb);
        __builtin_amdgcn_sched_barrier(0);
        RCBF_FAST_CHUNKS();
        RCBF_FAST_MID(hb);
        RCBF_FAST_CHUNKS();
        u0 = n0;
        u1 = n1;
        p2 = q2;
        p3 = q3;
#else
        RCBF_FAST_WALK_HEAD();
        CarsFastHead ha;
        cars_fast_head(prm, xs, a, st, u0, m, s, obs_c, ha);
        RCBF_FAST_MID(ha);
        RCBF_FAST_CHUNKS();
        RCBF_FAST_WALK_TAIL();
#endif
        if (__builtin_expect(fail_bits != 0, 0))
            __hip_atomic_fetch_or(failv, fail_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The steps the loop above did not run -- a wave with a lane out of the series' range, and a plan's odd last
    // step -- through the step k_safe_steps runs (safe_step_body: library sine outside the range, the same
    // stores), with the same walk of the table.
    const Stamps<false> stamps{};
#pragma nounroll
    while (left > 0) {
        --left;
        asm volatile("" : "+v"(epv), "+v"(failv));
        RCBF_FAST_WALK_HEAD();
        const float us[1] = {u0};
        bool rs = false;
        safe_step_body<RCBF_SOLVER_ACTIVE_SET, MODE, 1, false, false, true, false, false, 1>(
            prm, B, i, xv, auxv, stepv, epv, obsv, uv, rewv, costv, donev, (gptr<uint8_t>)nullptr,
            (gptr<int32_t>)nullptr, failv, auto_reset, seed, off, xs, a, st, us, m, s, true, epr, stamps, obs_stage[wid],
            nullptr, lane, &rs, obs_c);
        epr += rs ? 1u : 0u;  // a reset stored epr + 1
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        RCBF_FAST_WALK_TAIL();
    }
#undef RCBF_FAST_MID
#undef RCBF_FAST_CHUNKS
#undef RCBF_FAST_WALK_HEAD
#undef RCBF_FAST_WALK_TAIL
}

#define RCBF_SAFE_STEPS_FAST_INSTANTIATE(BS_)                                                                       \
    template __global__ void k_safe_steps_fast<BS_>(                                                                \
        int64_t, double* __restrict__, double* __restrict__, int32_t* __restrict__, const float* const* __restrict__, \
        uint32_t* __restrict__, const float* __restrict__, const float* __restrict__, float* __restrict__,          \
        float* __restrict__, float* __restrict__, float* __restrict__, uint8_t* __restrict__, uint8_t* __restrict__, \
        int32_t* __restrict__, int32_t*, int, uint64_t, int64_t, rcbf_params, int, int, int, int)

}  // namespace rcbf
