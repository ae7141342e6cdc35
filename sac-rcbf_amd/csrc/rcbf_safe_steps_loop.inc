    // rcbf_safe_steps_loop.inc -- the body of rcbf::k_safe_steps, rcbf::k_safe_steps_traj and
    // rcbf::k_safe_steps_term (rcbf_safe_step.hpp, which includes this file once in each, after `constexpr bool
    // TRAJ` and `#define RCBF_LOOP_TERM`, 1 in the last only): the prologue that loads env i's state, first
    // actions and priors, and the loop that runs env i's steps.  Not a header: it names the kernels' parameters
    // (B, x, ..., prm, prior_cols, n_u, steps, ju0) and template parameters (MODE, K, BS).
    // RCBF_LOOP_TERM is a preprocessor switch, not a third `if constexpr`: with the terminal pointer merely
    // declared in all three, the cars k_safe_steps_traj kernels came out with their prologue's register copies
    // in another order; this way the other two kernels' token stream is the one they had.
    using D = Dims<MODE, K>;
    constexpr int SOLVER = RCBF_SOLVER_ACTIVE_SET;
    constexpr bool WT = false;
    constexpr bool PLAIN = fused_plain<MODE, K, TRAJ>();
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
        if constexpr (TRAJ) *traj_stage_of<BS>(threadIdx.x >> 6) = traj_from_kernargs(0);  // ... and the row strides
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
#if RCBF_LOOP_TERM
    // the terminal observations' pointer, one more recorded pointer in an accumulation register
    static_assert(TRAJ && !PLAIN, "k_safe_steps_term: a trajectory kernel");
    gptr<float> termv = term_from_kernargs();
    asm volatile("" : "+a"(termv));
#endif
    // Everything loaded so far has arrived before the loop is entered (vmcnt(0); expcnt and lgkmcnt left
    // alone).  A wait for one of these loads inside the loop would be passed again in every step, where all
    // it can wait for is the last step's stores.
    __builtin_amdgcn_s_waitcnt(0x0f70);
    // Cars: what the loop carries from one step's tail to the next step's head (fused_carry, rcbf_safe_step.hpp).
    // obs_c: the fp32 observation row of env i's current state, which a step's layer reads through get_state
    // and which the step before it has just computed for its obs store; Gc, hc (the study form only): the
    // layer's raw rows for that state and the next action, built in that tail.  Derived here once from the
    // state just loaded, exactly as a step derives them (state_from_env, diff_rows), so a dispatch starts from
    // HBM alone.
    constexpr int CARRY = fused_carry<MODE>();
    float obs_c[D::NO], Gc[D::M][D::N], hc[D::M];
    if constexpr (CARRY != 0) {
        double o[D::NO];
        env_obs<MODE>(xs, o);
#pragma unroll
        for (int k = 0; k < D::NO; ++k) obs_c[k] = (float)o[k];
        if constexpr (CARRY == 2) {
            float s32[D::NS];
            state_from_obs32<MODE>(obs_c, s32);
            diff_rows<MODE, K>(prm, s32, us, m, s, Gc, hc, nullptr);
        }
    }
#pragma nounroll
    while (leftv > 0) {
        RCBF_OPAQUE_V();  // every step: nothing derived from them is loop-invariant to the compiler
#if RCBF_LOOP_TERM
        asm volatile("" : "+a"(termv));
#endif
        // The plain cars loop has no scalar register to spare (with the rows carried too, RCBF_FUSED_CARRY == 2,
        // it spilled four): the two pointers that only a reset and a failed solve use, as per-lane values (no
        // instruction).  Their null tests and env i's addresses are then worked out where those rare paths
        // need them, instead of standing in scalar registers over the whole step.
        if constexpr (PLAIN && CARRY != 0) asm volatile("" : "+v"(epv), "+v"(failv));
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
        constexpr bool OBS_PLAIN = TRAJ && RCBF_TRAJ_OBS_PLAIN != 0;  // study switch (rcbf_safe_step.hpp)
#if RCBF_LOOP_TERM
        safe_step_body<SOLVER, MODE, K, false, WT, true, OBS_SC1, OBS_PLAIN, CARRY, true>(
            prm_j, Bv, i, xv, auxv, stepv, epv, obsv, uv, rewv, costv, donev, goalv, statv, failv, arv, seedv, offv, xs,
            a, st, us, m, s, epv != nullptr, epr, stamps, obs_stage[widv], nullptr, lanev, &rs, CARRY ? obs_c : nullptr,
            CARRY ? Gc : nullptr, CARRY ? hc : nullptr, CARRY ? un : nullptr, termv);
#else
        safe_step_body<SOLVER, MODE, K, false, WT, true, OBS_SC1, OBS_PLAIN, CARRY>(
            prm_j, Bv, i, xv, auxv, stepv, epv, obsv, uv, rewv, costv, donev, goalv, statv, failv, arv, seedv, offv, xs,
            a, st, us, m, s, epv != nullptr, epr, stamps, obs_stage[widv], nullptr, lanev, &rs, CARRY ? obs_c : nullptr, CARRY ? Gc : nullptr, CARRY ? hc : nullptr,
            CARRY ? un : nullptr);
#endif
        epr += rs ? 1u : 0u;  // a reset stored epr + 1
        // this step's chunk reads of obs_stage stay ahead of the next step's writes to it (one wave's LDS
        // operations execute in order; this keeps the compiler from reordering them)
        __builtin_amdgcn_wave_barrier();
        // every step's stores are made in that step: without this the compiler, which sees in the plain form
        // that a step overwrites what the last one stored to aux, step, u, reward, cost and done, keeps those
        // in registers and stores them once after the loop (no instruction, no wait: a compiler barrier)
        asm volatile("" ::: "memory");
        if constexpr (TRAJ) {
            // every recorded output's pointer one row on, in place (64-bit; in the accumulation-register form
            // read, add, write back: nothing new lives across the step).  The mask and the pitch are read
            // again every step, as the parameter block is.
            TrajTail t;
            if constexpr (!PLAIN && K >= 8) {
                uint32_t voff = 0;
                asm volatile("" : "+v"(voff));
                t = *reinterpret_cast<const TrajTail*>(reinterpret_cast<const char*>(traj_stage_of<BS>(widv)) + voff);
            } else {
                uint32_t soff = 0;
                if constexpr (!PLAIN) asm volatile("" : "+s"(soff));
                t = traj_from_kernargs(soff);
            }
            const int64_t row = t.pitch;
            obsv += (t.mask & RCBF_TRAJ_OBS) ? row * D::NO : (int64_t)0;
            uv += (t.mask & RCBF_TRAJ_U) ? row * D::NU : (int64_t)0;
            rewv += (t.mask & RCBF_TRAJ_REWARD) ? row : (int64_t)0;
            costv += (t.mask & RCBF_TRAJ_COST) ? row : (int64_t)0;
            donev += (t.mask & RCBF_TRAJ_DONE) ? row : (int64_t)0;
            goalv += (t.mask & RCBF_TRAJ_GOAL_MET) ? row : (int64_t)0;
            statv += (t.mask & RCBF_TRAJ_STATUS) ? row : (int64_t)0;
#if RCBF_LOOP_TERM
            termv += (t.mask & RCBF_TRAJ_TERM_OBS) ? row * D::NO : (int64_t)0;
#endif
        }
#pragma unroll
        for (int c = 0; c < D::NU; ++c) us[c] = un[c];
        if constexpr (!PLAIN) asm volatile("" : "+s"(unext2));  // a scalar load's result, scalar till here
        unextv = unext2;
    }
#undef RCBF_OPAQUE_V
