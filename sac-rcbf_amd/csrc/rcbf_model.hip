// rcbf_model.hip -- model-based rollout step and the
// device replay buffer's ring scatter / row gather (8f row 4) + C-ABI.
//
// rcbf_model_step restates one k-step of generate_model_rollouts
// (rcbf_sac/generate_rollouts.py:24-77) for a batch of replay transitions:
//   state = get_state(obs); (mu, std) = predict_next_state(state, a, t)
//   (model prior + dt * disturbance mean, dt * disturbance std);
//   next_state = mu + std * z; next_obs = get_obs(next_state) (+ compass and
//   exp(-dist) for the unicycle); reward, done -> mask; next_t = t + dt.
// All fp64 like the reference's numpy, with FMA contraction off so the
// products round as numpy's do.
#include "rcbf_common.hpp"

using namespace rcbf;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The workgroup's rows (W elements of T each, row-major, rows row0 .. row0 + nrows) through LDS, so the
// global accesses are whole coalesced 16-B lane vectors; a row per lane would put the lanes W sizeof(T)
// bytes apart, each of its W load instructions touching a line per 1-2 lanes.  16-B accesses when the block's first element is 16-B aligned (a tensor's own storage is;
// a sliced view may not be), element accesses otherwise; all of a thread's loads are issued before its
// LDS stores.  s: kBlock * W elements, 16-B aligned.
template <typename T, int W>
__device__ __forceinline__ void rows_in(const T* __restrict__ src, int64_t row0, int nrows, T* s) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* p = src + row0 * W;
    const int n = nrows * W, t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        constexpr int kIt = (kBlock * W / V + kBlock - 1) / kBlock;
        const int nv = n / V;
        u32x4 v[kIt];
#pragma unroll
        for (int j = 0; j < kIt; ++j) {
            const int e = t + j * kBlock;
            if (e < nv) v[j] = reinterpret_cast<const u32x4*>(p)[e];
        }
#pragma unroll
        for (int j = 0; j < kIt; ++j) {
            const int e = t + j * kBlock;
            if (e < nv) reinterpret_cast<u32x4*>(s)[e] = v[j];
        }
        if (t < n - nv * V) s[nv * V + t] = p[nv * V + t];
    } else {
        T v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int e = t + j * kBlock;
            if (e < n) v[j] = p[e];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int e = t + j * kBlock;
            if (e < n) s[e] = v[j];
        }
    }
}

template <typename T, int W>
__device__ __forceinline__ void rows_out(T* __restrict__ dst, int64_t row0, int nrows, const T* s) {
    constexpr int V = 16 / (int)sizeof(T);
    T* p = dst + row0 * W;
    const int n = nrows * W, t = threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        constexpr int kIt = (kBlock * W / V + kBlock - 1) / kBlock;
        const int nv = n / V;
#pragma unroll
        for (int j = 0; j < kIt; ++j) {
            const int e = t + j * kBlock;
            if (e < nv) reinterpret_cast<u32x4*>(p)[e] = reinterpret_cast<const u32x4*>(s)[e];
        }
        if (t < n - nv * V) p[nv * V + t] = s[nv * V + t];
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int e = t + j * kBlock;
            if (e < n) p[e] = s[e];
        }
    }
}

// get_state (dynamics.py:190-232), numpy fp64 path
template <int MODE>
__device__ __forceinline__ void model_state_from_obs(const double* o, double* xs) {
#pragma clang fp contract(off)
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
#pragma unroll
        for (int k = 0; k < 10; ++k) xs[k] = o[k] * ((k & 1) ? 30.0 : 100.0);
    } else {
        xs[0] = o[0];
        xs[1] = o[1];
        xs[2] = atan2(o[3], o[2]);
    }
}

// f(x, t) + g(x) u of the model prior (dynamics.py:125-188), the rate itself: DynamicsModel._f_plus_gu
// operation for operation, the `+ 0.0` of the zero f / gu entries included
template <int MODE>
__device__ __forceinline__ void model_prior_rate(const double* xs, const double* u, double t, double* F) {
#pragma clang fp contract(off)
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
        double pos[5], vel[5], acc[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            pos[c] = xs[2 * c];
            vel[c] = xs[2 * c + 1];
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            double vdes = 30.0;
            if (c == 0) vdes -= 10.0 * sin(0.2 * t);
            acc[c] = 4.0 * (vdes - vel[c]);
        }
        const double d01 = pos[0] - pos[1], d12 = pos[1] - pos[2], d24 = pos[2] - pos[4];
        acc[1] -= 20.0 * d01 * (d01 < 6.0 ? 1.0 : 0.0);
        acc[2] -= 20.0 * d12 * (d12 < 6.0 ? 1.0 : 0.0);
        acc[3] = 0.0;
        acc[4] -= 20.0 * d24 * (d24 < 13.0 ? 1.0 : 0.0);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            F[2 * c] = vel[c] + 0.0;
            F[2 * c + 1] = acc[c] + (c == 3 ? 50.0 * u[0] : 0.0);
        }
    } else {
        double s, c;
        sincos(xs[2], &s, &c);
        F[0] = 0.0 + c * u[0];
        F[1] = 0.0 + s * u[0];
        F[2] = 0.0 + u[1];
    }
}

// x + dt (f(x) + g(x) u) of the model prior (dynamics.py:60-105)
template <int MODE>
__device__ __forceinline__ void model_prior_next(const double* xs, const double* u, double t, double* nx) {
#pragma clang fp contract(off)
    constexpr int NS = Dims<MODE, 1>::NS;
    const double dt = 0.02;
    double F[NS];
    model_prior_rate<MODE>(xs, u, t, F);
#pragma unroll
    for (int k = 0; k < NS; ++k) nx[k] = xs[k] + dt * F[k];
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_model_step(rcbf_params prm, int64_t B, const double* __restrict__ obs,
                                                       const double* __restrict__ act, const double* __restrict__ t,
                                                       const float* __restrict__ mean, const float* __restrict__ stdv,
                                                       const double* __restrict__ z, uint64_t seed, uint64_t counter,
                                                       double* __restrict__ next_obs, double* __restrict__ reward,
                                                       double* __restrict__ mask, double* __restrict__ next_t) {
#pragma clang fp contract(off)
    using D = Dims<MODE, 1>;
    constexpr int NS = D::NS, NO = D::NO, NU = D::NU;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    const double dt = 0.02;
    double o[NO], xs[NS], u[NU], nx[NS];
#pragma unroll
    for (int k = 0; k < NO; ++k) o[k] = obs[i * NO + k];
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = act[i * NU + c];
    const double ti = t ? t[i] : 0.0;
    model_state_from_obs<MODE>(o, xs);
    model_prior_next<MODE>(xs, u, ti, nx);
    // disturbance: GP (mean, std) or the zero-mean MAX_STD prior (dynamics.py:381-384)
    double zz[NS];
    if (z) {
#pragma unroll
        for (int k = 0; k < NS; ++k) zz[k] = z[i * NS + k];
    } else {  // N(0,1) from Philox4x32-10 keyed by (seed, row, counter, call q): one call = 4 words = 2
              // Box-Muller pairs on 24-bit uniforms with the hardware fp32 log2 / sin / cos (as the envs'
              // reset draw, normal_draw); statistically N(0, 1), |z| <= 5.8 (r04: cars 5 fp64 pairs -> 3 calls)
#pragma unroll
        for (int q = 0; q < (NS + 3) / 4; ++q) {
            uint32_t cc[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)counter, (uint32_t)q};
            philox4x32_10(cc, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float zc, zs;
                box_muller_pair(cc[2 * h], cc[2 * h + 1], zc, zs);
                const int k = 4 * q + 2 * h;
                if (k < NS) zz[k] = (double)zc;
                if (k + 1 < NS) zz[k + 1] = (double)zs;
            }
        }
    }
    double ns[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double m = mean ? (double)mean[i * NS + k] : 0.0;
        // MAX_STD as numpy fp64 (dynamics.py:24,381-384)
        const double prior = (MODE == RCBF_MODE_UNICYCLE || (k & 1)) ? 0.2 : 0.0;
        const double sd = stdv ? (double)stdv[i * NS + k] : prior;
        const double mu = nx[k] + dt * m;      // next_state_batch += dt * pred_mean
        ns[k] = mu + (dt * sd) * zz[k];        // np.random.normal(mu, dt * pred_std)
    }
    double r, msk;
    const double tn = ti + dt;
    if constexpr (MODE == RCBF_MODE_SIMULATED_CARS) {
#pragma unroll
        for (int k = 0; k < 10; ++k)  // correctly rounded x / d in 3 FMAs (div_const), numpy's x / d bit for bit
            next_obs[i * NO + k] = (k & 1) ? div_const(ns[k], 30.0, 1.0 / 30.0) : div_const(ns[k], 100.0, 1.0 / 100.0);
        r = -5.0 * fabs(u[0] * u[0]) / 300.0;     // generate_rollouts.py:62
        msk = (tn >= 300.0 * 0.02) ? 0.0 : 1.0;   // :65-66
    } else {
        double s, c;
        sincos(ns[2], &s, &c);
        const double g0 = 2.5 - ns[0], g1 = 2.5 - ns[1];
        const double d = sqrt(g0 * g0 + g1 * g1);
        double c0 = g0 * c + g1 * s;       // goal_rel @ R(theta)  (:41)
        double c1 = g0 * (-s) + g1 * c;
        const double nrm = sqrt(c0 * c0 + c1 * c1) + 0.001;
        c0 = c0 / nrm;
        c1 = c1 / nrm;
        double* nw = &next_obs[i * NO];
        nw[0] = ns[0];
        nw[1] = ns[1];
        nw[2] = c;
        nw[3] = s;
        nw[4] = c0;
        nw[5] = c1;
        nw[6] = exp(-d);
        const double dprev = -log(o[NO - 1]);
        const bool goal = d <= 0.3;
        r = (dprev - d) * 1.0 + (goal ? 1.0 : 0.0);  // :47
        r = r + 1.0 * (goal ? 1.0 : 0.0);          // :51, the goal bonus counted twice
        msk = goal ? 0.0 : 1.0;
    }
    reward[i] = r;
    mask[i] = msk;
    if (next_t) next_t[i] = tn;
}

// DynamicsModel.predict_next_state (dynamics.py:60-105) on device rows:
// next = x + dt (f(x) + g(x) u) [+ dt * mean when use_gps], std_out = dt * std
// (zeros without use_gps), next_t = t + dt.  The disturbance (mean, std) is
// the fitted GP's posterior (f32, rcbf_gp_predict) or, when null, the
// zero-mean MAX_STD prior (dynamics.py:381-384).  fp64 rows, contraction off:
// the same roundings as the reference's numpy.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_predict_next_state(int64_t B, const double* __restrict__ x,
                                                               const double* __restrict__ act,
                                                               const double* __restrict__ t,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, int use_gps,
                                                               double* __restrict__ next_x,
                                                               double* __restrict__ std_out,
                                                               double* __restrict__ next_t) {
#pragma clang fp contract(off)
    using D = Dims<MODE, 1>;
    constexpr int NS = D::NS, NU = D::NU;
    // the cars' 80-B rows (x in; next_x, std_out out; 40-B mean / std in) go through LDS (rows_in /
    // rows_out): 11.1 -> 8.0 us at B = 65 536 (r05zb); the unicycle's 24-B rows stay per lane (3.8 us
    // per lane, 4.0 staged), as do the model step's rows (6.2 us per lane, 6.4 staged: its time is the
    // fp64 sin / Philox chain, not the access pattern)
    constexpr bool kStage = NS * (int)sizeof(double) >= 64;
    constexpr int kS = kStage ? kBlock * NS / 2 + 1 : 1, kM = kStage ? kBlock * NS / 4 + 1 : 1;
    __shared__ u32x4 s_x[kS], s_sd[kS], s_ms[2][kM];
    double* sx = reinterpret_cast<double*>(s_x);
    double* sd_rows = reinterpret_cast<double*>(s_sd);
    const int64_t row0 = (int64_t)blockIdx.x * kBlock;
    const int nrows = (int)min((int64_t)kBlock, B - row0);
    const int64_t i = row0 + threadIdx.x;
    const bool live = threadIdx.x < nrows;
    if constexpr (!kStage) {
        if (!live) return;
    } else {
        rows_in<double, NS>(x, row0, nrows, sx);
        if (use_gps && mean) rows_in<float, NS>(mean, row0, nrows, reinterpret_cast<float*>(s_ms[0]));
        if (use_gps && stdv) rows_in<float, NS>(stdv, row0, nrows, reinterpret_cast<float*>(s_ms[1]));
    }
    const double dt = 0.02;
    double xs[NS], u[NU], nx[NS];
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = live ? act[i * NU + c] : 0.0;
    const double ti = (t && live) ? t[i] : 0.0;
    if constexpr (kStage) __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) xs[k] = kStage ? sx[threadIdx.x * NS + k] : x[i * NS + k];
    model_prior_next<MODE>(xs, u, ti, nx);
    const float* sm = kStage ? reinterpret_cast<const float*>(s_ms[0]) + threadIdx.x * NS : mean + i * NS;
    const float* ss = kStage ? reinterpret_cast<const float*>(s_ms[1]) + threadIdx.x * NS : stdv + i * NS;
    if constexpr (kStage) __syncthreads();  // every thread has read its x row: the buffer takes the next_x rows
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double sd = 0.0;
        if (use_gps) {
            const double m = mean ? (double)sm[k] : 0.0;
            const double prior = (MODE == RCBF_MODE_UNICYCLE || (k & 1)) ? 0.2 : 0.0;  // MAX_STD
            sd = stdv ? (double)ss[k] : prior;
            nx[k] = nx[k] + dt * m;  // next_state_batch += dt * pred_mean
        }
        if constexpr (kStage) {
            sx[threadIdx.x * NS + k] = nx[k];
            sd_rows[threadIdx.x * NS + k] = dt * sd;
        } else {
            next_x[i * NS + k] = nx[k];
            std_out[i * NS + k] = dt * sd;
        }
    }
    if (next_t && live) next_t[i] = ti + dt;
    if constexpr (kStage) {
        __syncthreads();
        rows_out<double, NS>(next_x, row0, nrows, sx);
        rows_out<double, NS>(std_out, row0, nrows, sd_rows);
    }
}

// Replay ring (rcbf_sac/replay_memory.py:12-32): records are rows of W f64.
__global__ void __launch_bounds__(256) k_ring_scatter(double* __restrict__ ring, int64_t cap, int64_t W, int64_t pos,
                                                      const double* __restrict__ src, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * W) return;
    const int64_t r = e / W, c = e - r * W;
    ring[((pos + r) % cap) * W + c] = src[e];
}

__global__ void __launch_bounds__(256) k_gather_rows(double* __restrict__ dst, const double* __restrict__ ring,
                                                     int64_t W, const int64_t* __restrict__ idx, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * W) return;
    const int64_t r = e / W, c = e - r * W;
    dst[e] = ring[idx[r] * W + c];
}

// `n` doubles from this wave's LDS block (s) to ring[dst0 ...], one contiguous run, as whole 16-B lane vectors
// wherever the destination allows it: a run that starts on an odd double (records are W doubles, W odd) stores
// that one double alone, the aligned pairs follow (two 8-B LDS reads, one dwordx4 `nt` store, pair p by lane
// p % 64), and an odd double left at the end leaves alone too.  Nothing of the ring is read.
__device__ __forceinline__ void run_out(double* __restrict__ ring, int64_t dst0, const double* s, int n, int lane) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    if (n <= 0) return;
    double* const p = ring + dst0;
    const int head = (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1);
    const int npair = (n - head) >> 1;
    for (int q = lane; q < npair; q += 64) {
        const d2 v = {s[head + 2 * q], s[head + 2 * q + 1]};
        __builtin_nontemporal_store(v, reinterpret_cast<d2*>(p + head + 2 * q));
    }
    if (lane == 0 && head) __builtin_nontemporal_store(s[0], p);
    if (lane == 1 && ((n - head) & 1)) __builtin_nontemporal_store(s[n - 1], p + n - 1);
}

// a trajectory's observation row of NO floats (`nt`, read once): 8-byte pairs where rows are 8-byte aligned
// (cars, 40 B), dwords otherwise (28 B)
template <int NO>
__device__ __forceinline__ void load_obs_row(const float* __restrict__ row, float* o) {
    if constexpr (NO % 2 == 0) {
        typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int k = 0; k < NO / 2; ++k) {
            const f2 v = __builtin_nontemporal_load(reinterpret_cast<const f2*>(row) + k);
            o[2 * k] = v.x;
            o[2 * k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NO; ++k) o[k] = ld_in(&row[k]);
    }
}

// rcbf_traj_pack_replay_f64: the K x B transitions of a trajectory plan as packed replay records, written
// straight into the ring.  One env per lane, a wave per workgroup; the lane that owns env i walks steps
// [j0, j1) = blockIdx.y's chunk of `chunk` steps, carrying env i's episode-step count (recomputed from
// step0 and the done bytes of the steps before j0: one byte per step, against ~300 of a transition) and the
// row obs[j - 1][i], which is next_obs of one record and obs_prev of the next (loaded once).  Every input is
// read once (`nt`); a wave's 64 rows of obs[j] are one contiguous block of memory.
// Output: the wave's records of step j, r = j B + i, are consecutive slots of the ring, so its 64 W doubles
// are ONE run of memory unless the ring wraps inside it (then two).  The lanes write their records to LDS
// (a row per lane, W odd: no bank conflict), and the block leaves as 16-B lane vectors (run_out) instead of
// W strided 8-B stores per lane.  Transitions r < skip (= K B - capacity when that is positive) are the
// ones sequential pushes would have overwritten: not written, so no slot is written twice and at most
// `cap` consecutive slots are written per wave and step -- one wrap at the most.
template <int NO, int NU>
__global__ void __launch_bounds__(64) k_traj_pack_replay(double* __restrict__ ring, int64_t cap, int64_t pos,
                                                         int64_t skip, int64_t B, int K, int64_t P,
                                                         const float* __restrict__ obs0,
                                                         const int32_t* __restrict__ step0,
                                                         const float* __restrict__ obs,
                                                         const float* __restrict__ term,
                                                         const float* __restrict__ u,
                                                         const float* __restrict__ reward,
                                                         const uint8_t* __restrict__ done, int max_steps, double dt,
                                                         int auto_reset, int chunk) {
    constexpr int W = 2 * NO + NU + 4;
    __shared__ __attribute__((aligned(16))) double stage[64 * W];
    const int lane = threadIdx.x;
    const int64_t wbase = (int64_t)blockIdx.x * 64;
    const int64_t i = wbase + lane;
    const bool live = i < B;
    const int nl = (int)(B - wbase < 64 ? B - wbase : 64);  // this wave's envs
    const int j0 = (int)blockIdx.y * chunk;
    const int j1 = j0 + chunk < K ? j0 + chunk : K;
    int c = 0;
    float prev[NO];
#pragma unroll
    for (int k = 0; k < NO; ++k) prev[k] = 0.0f;
    if (live) {
        c = ld_in(&step0[i]);
        for (int j = 0; j < j0; ++j) {  // the count at the chunk's first step
            const bool dn = ld_in(&done[(int64_t)j * P + i]) != 0;
            c = (dn && auto_reset) ? 0 : c + 1;
        }
        load_obs_row<NO>(j0 == 0 ? obs0 + i * NO : obs + ((int64_t)(j0 - 1) * P + i) * NO, prev);
    }
    for (int j = j0; j < j1; ++j) {
        if (live) {
            const int64_t e = (int64_t)j * P + i;
            float cur[NO], nx[NO], uj[NU];
            load_obs_row<NO>(obs + e * NO, cur);
#pragma unroll
            for (int k = 0; k < NU; ++k) uj[k] = ld_in(&u[e * NU + k]);
            const float rw = ld_in(&reward[e]);
            const bool dn = ld_in(&done[e]) != 0;
#pragma unroll
            for (int k = 0; k < NO; ++k) nx[k] = cur[k];
            if (dn && auto_reset && term) load_obs_row<NO>(term + e * NO, nx);  // rare: the episode's last observation
            const int ep = c + 1;
            double* const rec = stage + lane * W;
#pragma unroll
            for (int k = 0; k < NO; ++k) rec[k] = (double)prev[k];
#pragma unroll
            for (int k = 0; k < NU; ++k) rec[NO + k] = (double)uj[k];
            rec[NO + NU] = (double)rw;
#pragma unroll
            for (int k = 0; k < NO; ++k) rec[NO + NU + 1 + k] = (double)nx[k];
            rec[2 * NO + NU + 1] = ep == max_steps ? 1.0 : 1.0 - (dn ? 1.0 : 0.0);
            rec[2 * NO + NU + 2] = (double)ep * dt;
            rec[2 * NO + NU + 3] = (double)(ep + 1) * dt;
            c = (dn && auto_reset) ? 0 : ep;
#pragma unroll
            for (int k = 0; k < NO; ++k) prev[k] = cur[k];
        }
        __syncthreads();  // one wave: the records are in LDS
        // the wave's kept records [qa, nl) of this step, at slots sa, sa + 1, ... (mod cap)
        const int64_t r0 = (int64_t)j * B + wbase;
        const int qa = skip > r0 ? (skip - r0 < nl ? (int)(skip - r0) : nl) : 0;
        const int kept = nl - qa;
        if (kept > 0) {
            const int64_t sa = (pos + r0 + qa) % cap;
            const int n1 = cap - sa < kept ? (int)(cap - sa) : kept;
            run_out(ring, sa * W, stage + qa * W, n1 * W, lane);
            run_out(ring, 0, stage + (qa + n1) * W, (kept - n1) * W, lane);
        }
        __syncthreads();  // ... and read, before the next step's records overwrite them
    }
}

// rcbf_traj_pack_gp_f64: the transitions of a trajectory plan that the reference's loop hands to
// DynamicsModel.append_transition (main.py:110-113: every `every`-th episode step), as rows (x, d) of the GP's
// disturbance dataset, compacted.  Which transitions are selected depends on the done bytes, so the work is
// three launches on one stream: k_traj_gp_count (the selected lanes of each (step, wave), from a ballot),
// k_traj_gp_scan (their exclusive prefix sum in step-major, wave-minor order: the slot of every wave's first
// selected row of every step; one workgroup, fixed order, no atomics) and k_traj_pack_gp (the rows).

// An env's episode-step count along the plan: c before a step, and r = c mod `every` carried beside it so that
// "e = c + 1 is a multiple of `every`" costs no division per step.  The recurrence of k_traj_pack_replay.
struct EpisodeStep {
    int c, r;
    __device__ __forceinline__ void start(int c0, int every) {
        c = c0;
        r = c0 % every;
    }
    // one step; returns e, and in `sel` whether the reference appends this transition
    __device__ __forceinline__ int step(bool reset, int every, bool& sel) {
        const int e = c + 1;
        r = r + 1 == every ? 0 : r + 1;
        sel = r == 0;
        c = reset ? 0 : e;
        if (reset) r = 0;
        return e;
    }
    // the steps [0, j_end) of env i, from the done bytes alone: only the last reset before j_end matters (the
    // count is the steps since it, or c0 + j_end without one), so the bytes are loaded 16 at a time, all 16 in
    // flight together, and compared -- a load's latency per 16 steps instead of per step
    __device__ __forceinline__ void walk(const uint8_t* __restrict__ done, int64_t P, int64_t i, int j_end,
                                         int auto_reset, int every) {
        if (j_end <= 0) return;
        int last = -1;
        if (auto_reset) {
            int j = 0;
            for (; j + 16 <= j_end; j += 16) {
                uint8_t b[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) b[k] = ld_in(&done[(int64_t)(j + k) * P + i]);
#pragma unroll
                for (int k = 0; k < 16; ++k) last = b[k] ? j + k : last;
            }
            for (; j < j_end; ++j) last = ld_in(&done[(int64_t)j * P + i]) ? j : last;
        }
        start(last >= 0 ? j_end - 1 - last : c + j_end, every);
    }
};

// counts[j waves + w] = selected transitions among wave w's envs at step j.  Grid and chunks as k_traj_pack_gp.
__global__ void __launch_bounds__(64) k_traj_gp_count(int64_t* __restrict__ counts, int64_t B, int K, int64_t P,
                                                      const int32_t* __restrict__ step0,
                                                      const uint8_t* __restrict__ done, int auto_reset, int every,
                                                      int chunk) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool live = i < B;
    const int j0 = (int)blockIdx.y * chunk;
    const int j1 = j0 + chunk < K ? j0 + chunk : K;
    EpisodeStep ep;
    ep.start(live ? ld_in(&step0[i]) : 0, every);
    if (live) ep.walk(done, P, i, j0, auto_reset, every);
    for (int j = j0; j < j1; j += 8) {  // 8 steps' bytes in flight together
        uint8_t b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = (live && j + k < j1) ? ld_in(&done[(int64_t)(j + k) * P + i]) : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (j + k < j1) {  // (wave-uniform)
                bool sel = false;
                if (live) ep.step(b[k] != 0 && auto_reset, every, sel);
                const unsigned long long m = __ballot(sel);
                if (lane == 0) counts[(int64_t)(j + k) * gridDim.x + blockIdx.x] = (int64_t)__popcll(m);
            }
        }
    }
}

// v[0 .. n) (counts) -> their exclusive prefix sums, in place, and v[n] = the total; count_out = {total,
// min(total, keep_last)}.  ONE workgroup: tiles of 1024 x 16 consecutive elements (a thread's 16 are contiguous,
// all loaded before any is used), a wave scan of the thread sums, the 16 wave sums through LDS, the tiles'
// total carried.  Same order of additions in every run; n is K x waves, 20 480 at B = 65 536, K = 20.
__global__ void __launch_bounds__(1024) k_traj_gp_scan(int64_t* __restrict__ v, int64_t n, int64_t keep_last,
                                                       int64_t* __restrict__ count_out) {
    constexpr int kIt = 16;
    __shared__ long long wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += 1024 * kIt) {
        const int64_t e0 = base + (int64_t)threadIdx.x * kIt;
        long long a[kIt];
#pragma unroll
        for (int k = 0; k < kIt; ++k) a[k] = e0 + k < n ? (long long)v[e0 + k] : 0;
        long long tsum = 0;
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
            const long long t = a[k];
            a[k] = tsum;
            tsum += t;
        }
        long long inc = tsum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long s = wsum[w];
            if (w < wave) before += s;
            total += s;
        }
        const long long ex = carry + before + (inc - tsum);
#pragma unroll
        for (int k = 0; k < kIt; ++k)
            if (e0 + k < n) v[e0 + k] = (int64_t)(ex + a[k]);
        carry += total;
        __syncthreads();  // the wave sums are read before the next tile's replace them
    }
    if (threadIdx.x == 0) {
        v[n] = (int64_t)carry;
        count_out[0] = (int64_t)carry;
        count_out[1] = (int64_t)(carry < keep_last ? carry : keep_last);
    }
}

// The pack pass.  One env per lane, a wave per workgroup, steps [j0, j1) = blockIdx.y's chunk, the lane carrying
// its env's step count and the row obs[j - 1][i] (x' of one transition, x of the next: loaded once), as
// k_traj_pack_replay.  At step j the wave's selected lanes are ranked by a ballot; lane of rank q forms
//   x = get_state(obs_prev), x' = get_state(next_obs), F = f(x, e dt) + g(x) u, d = ((x' - x) - dt F) / dt
// (fp64, the numpy path's order: dynamics.py:190-232, :263-303) and writes both rows at row q of the wave's LDS
// block.  The wave's rows of a step are rows offs[j waves + w] ... of the compacted result, ONE contiguous run
// of each output, stored as 16-B lane vectors (run_out).  Only the last keep_last selected rows are kept: rows
// before skip = n_sel - keep_last are not written, a workgroup whose chunk lies wholly before it ends at once,
// and one that straddles it starts at the first step that has a kept row.
template <int MODE>
__global__ void __launch_bounds__(64) k_traj_pack_gp(double* __restrict__ state_out, double* __restrict__ dist_out,
                                                     const int64_t* __restrict__ offs, int64_t keep_last, int64_t B,
                                                     int K, int64_t P, const float* __restrict__ obs0,
                                                     const int32_t* __restrict__ step0,
                                                     const float* __restrict__ obs, const float* __restrict__ term,
                                                     const float* __restrict__ u, const uint8_t* __restrict__ done,
                                                     double dt, int auto_reset, int every, int chunk) {
#pragma clang fp contract(off)
    using D = Dims<MODE, 1>;
    constexpr int NO = D::NO, NU = D::NU, NS = D::NS;
    __shared__ __attribute__((aligned(16))) double stage_x[64 * NS];
    __shared__ __attribute__((aligned(16))) double stage_d[64 * NS];
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, waves = gridDim.x;
    const int64_t i = w * 64 + lane;
    const bool live = i < B;
    const int j0 = (int)blockIdx.y * chunk;
    const int j1 = j0 + chunk < K ? j0 + chunk : K;
    const int64_t n_sel = offs[(int64_t)K * waves];
    const int64_t skip = n_sel > keep_last ? n_sel - keep_last : 0;
    // rows selected up to and including this wave's of step j
    auto end_of = [&](int j) { return offs[(int64_t)j * waves + w + 1]; };
    if (end_of(j1 - 1) <= skip) return;  // (wave-uniform) nothing of this chunk is kept, or nothing is selected
    int ja = j0;
    if (skip > 0) {  // the first step of the chunk with a kept row: the offsets are monotone
        int hi = j1 - 1;
        while (ja < hi) {
            const int mid = (ja + hi) >> 1;
            if (end_of(mid) > skip)
                hi = mid;
            else
                ja = mid + 1;
        }
    }
    EpisodeStep ep;
    ep.start(live ? ld_in(&step0[i]) : 0, every);
    float prev[NO];
#pragma unroll
    for (int k = 0; k < NO; ++k) prev[k] = 0.0f;
    if (live) {
        ep.walk(done, P, i, ja, auto_reset, every);
        load_obs_row<NO>(ja == 0 ? obs0 + i * NO : obs + ((int64_t)(ja - 1) * P + i) * NO, prev);
    }
    for (int j = ja; j < j1; ++j) {
        const int64_t e = (int64_t)j * P + i;
        float cur[NO], uj[NU];
        bool sel = false, reset = false;
        int es = 0;
        if (live) {
            load_obs_row<NO>(obs + e * NO, cur);
#pragma unroll
            for (int k = 0; k < NU; ++k) uj[k] = ld_in(&u[e * NU + k]);
            reset = ld_in(&done[e]) != 0 && auto_reset;
            es = ep.step(reset, every, sel);
        }
        const unsigned long long m = __ballot(sel);
        const int n_w = __popcll(m);
        if (sel) {
            const int q = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            float nx[NO];
#pragma unroll
            for (int k = 0; k < NO; ++k) nx[k] = cur[k];
            if (reset) load_obs_row<NO>(term + e * NO, nx);  // rare: the episode's last observation
            double o[NO], x[NS], xn[NS], ud[NU], F[NS];
#pragma unroll
            for (int k = 0; k < NO; ++k) o[k] = (double)prev[k];
            model_state_from_obs<MODE>(o, x);
#pragma unroll
            for (int k = 0; k < NO; ++k) o[k] = (double)nx[k];
            model_state_from_obs<MODE>(o, xn);
#pragma unroll
            for (int k = 0; k < NU; ++k) ud[k] = (double)uj[k];
            model_prior_rate<MODE>(x, ud, (double)es * dt, F);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                stage_x[q * NS + k] = x[k];
                stage_d[q * NS + k] = ((xn[k] - x[k]) - dt * F[k]) / dt;
            }
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < NO; ++k) prev[k] = cur[k];
        }
        __syncthreads();  // one wave: the rows are in LDS
        // the wave's n_w rows of this step are rows g0, g0 + 1, ... of the selection; kept from row `skip` on
        const int64_t g0 = offs[(int64_t)j * waves + w];
        const int qa = skip > g0 ? (skip - g0 < n_w ? (int)(skip - g0) : n_w) : 0;
        const int kept = n_w - qa;
        if (kept > 0) {
            const int64_t dst = (g0 + qa - skip) * NS;
            run_out(state_out, dst, stage_x + qa * NS, kept * NS, lane);
            run_out(dist_out, dst, stage_d + qa * NS, kept * NS, lane);
        }
        __syncthreads();  // ... and read, before the next step's rows overwrite them
    }
}

// Steps per workgroup of the trajectory packers (one wave of envs per workgroup, K steps): the whole plan where
// the batch alone fills the chip (8 waves a CU), shorter chunks (each lane then first re-derives its step count
// from the done bytes before its chunk) where it does not.
inline int traj_steps_per_workgroup(int64_t waves, int K) {
    const int64_t want = (int64_t)num_cus() * 8;
    int64_t parts = waves >= want ? 1 : (want + waves - 1) / waves;
    if (parts > K) parts = K;
    if (parts > 65535) parts = 65535;
    return (int)((K + parts - 1) / parts);
}

// rcbf_traj_episode_stats_f64: the reference loop's episode bookkeeping (main.py:98-101: episode_reward +=
// reward, episode_cost += info['cost'], episode_steps += 1; :140-144: the line an episode that ends logs) over
// the (K, P) reward, cost and done arrays of a trajectory plan.  Which (step, env) pairs end an episode depends
// on the done bytes alone, so the work is the three launches of the GP packer: k_traj_ep_count (the lanes of
// each (step, wave) that end one, from a ballot), k_traj_gp_scan as it stands (their exclusive prefix sum,
// step-major, wave-minor: the record index of every wave's first episode of every step) and k_traj_ep_pack.

// counts[j waves + w] = envs of wave w whose episode ends at step j.  No state runs from step to step (a done
// byte ends an episode whatever the sums are), so blockIdx.y's chunk of steps starts cold; 8 steps' bytes are in
// flight together, as in k_traj_gp_count.
__global__ void __launch_bounds__(64) k_traj_ep_count(int64_t* __restrict__ counts, int64_t B, int K, int64_t P,
                                                      const uint8_t* __restrict__ done, int auto_reset, int chunk) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool live = i < B;
    const int j0 = (int)blockIdx.y * chunk;
    const int j1 = j0 + chunk < K ? j0 + chunk : K;
    for (int j = j0; j < j1; j += 8) {
        uint8_t b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = (live && j + k < j1) ? ld_in(&done[(int64_t)(j + k) * P + i]) : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (j + k < j1) {  // (wave-uniform)
                const unsigned long long m = __ballot(b[k] != 0 && auto_reset);
                if (lane == 0) counts[(int64_t)(j + k) * gridDim.x + blockIdx.x] = (int64_t)__popcll(m);
            }
        }
    }
}

// kEpSteps steps of one env's reward, cost and done from step j on: row-coalesced `nt` loads (a wave's 64
// values of a step are one run of memory), all issued before any is used, and none of them conditional: a lane
// past B loads env B - 1's values and a step past K step K - 1's (the same lines again), to be ignored.
constexpr int kEpSteps = 8;
template <bool COST>
struct EpisodeBlock {
    float rw[kEpSteps], cs[kEpSteps];
    uint8_t dn[kEpSteps];
    __device__ __forceinline__ void load(const float* __restrict__ reward, const float* __restrict__ cost,
                                         const uint8_t* __restrict__ done, int64_t P, int64_t i, int j, int K) {
#pragma unroll
        for (int k = 0; k < kEpSteps; ++k) {
            const int64_t e = (int64_t)(j + k < K ? j + k : K - 1) * P + i;
            rw[k] = ld_in(&reward[e]);
            if constexpr (COST) cs[k] = ld_in(&cost[e]);
            dn[k] = ld_in(&done[e]);
        }
    }
};

// The pack pass.  One env per lane, a wave per workgroup, the lane carrying its env's return R, cost C and
// episode-step count c in registers over all K steps (each is the sum of everything before it: the additions
// are made in step order, fp32 widened exactly, so every output is bit-reproducible from the inputs).  The
// loads run a block of kEpSteps steps ahead of the adds: the next block's are issued before this block's first
// value is used, so a lane waits for a load round trip once per block at the most, not once per step.  At a step
// where lanes end an episode they are ranked by a ballot; the lane of rank q owns record offs[j waves + w] + q
// and stores its five values there if that is below max_rows -- the stores of one field from one wave and step
// are one contiguous run.  Episode ends are sparse: plain per-lane stores, no LDS staging.
template <bool COST>
__global__ void __launch_bounds__(64) k_traj_ep_pack(int32_t* __restrict__ ep_env, int32_t* __restrict__ ep_step,
                                                     int32_t* __restrict__ ep_len, double* __restrict__ ep_return,
                                                     double* __restrict__ ep_cost, const int64_t* __restrict__ offs,
                                                     int64_t max_rows, int64_t B, int K, int64_t P,
                                                     const float* __restrict__ reward,
                                                     const float* __restrict__ cost,
                                                     const uint8_t* __restrict__ done,
                                                     const double* __restrict__ carry_in,
                                                     const int32_t* __restrict__ len_in,
                                                     double* __restrict__ carry_out, int32_t* __restrict__ len_out,
                                                     int auto_reset) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x;
    const int64_t w = blockIdx.x, waves = gridDim.x;
    const int64_t i = w * 64 + lane;
    const bool live = i < B;
    const int64_t il = live ? i : B - 1;  // the env whose values this lane loads
    const bool on = live && auto_reset;   // this lane's done bytes end episodes
    double R = 0.0, C = 0.0;
    int c = 0;
    if (carry_in) {  // (the oldest loads: complete when the first block's are)
        const double2 v = ld_in2(carry_in + 2 * il);
        R = v.x;
        C = v.y;
    }
    if (len_in) c = ld_in(&len_in[il]);
    // the steps [j, j + kEpSteps) below K, their values in `blk`
    auto walk = [&](const EpisodeBlock<COST>& blk, int j) {
#pragma unroll
        for (int k = 0; k < kEpSteps; ++k) {
            if (j + k >= K) break;  // (wave-uniform)
            R = R + (double)blk.rw[k];
            if constexpr (COST) C = C + (double)blk.cs[k];
            const int e = c + 1;
            const bool end = (blk.dn[k] != 0) & on;
            const unsigned long long m = __ballot(end);
            if (end) {
                const int q =
                    (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                const int64_t slot = offs[(int64_t)(j + k) * waves + w] + q;
                if (slot < max_rows) {
                    ep_env[slot] = (int32_t)i;
                    ep_step[slot] = j + k;
                    ep_len[slot] = e;
                    ep_return[slot] = R;
                    ep_cost[slot] = C;
                }
            }
            R = end ? 0.0 : R;
            C = end ? 0.0 : C;
            c = end ? 0 : e;
        }
    };
    // two blocks in turn, each reloaded as soon as it is walked: no copy between them, and a load is never
    // conditional (past K it repeats row K - 1), so the wait before a block's first value leaves the other
    // block's loads in flight
    EpisodeBlock<COST> a, b;
    a.load(reward, cost, done, P, il, 0, K);
    for (int j = 0; j < K; j += 2 * kEpSteps) {
        b.load(reward, cost, done, P, il, j + kEpSteps, K);
        walk(a, j);
        a.load(reward, cost, done, P, il, j + 2 * kEpSteps, K);
        walk(b, j + kEpSteps);
    }
    if (live && carry_out) {
        const d2 v = {R, C};
        __builtin_nontemporal_store(v, reinterpret_cast<d2*>(carry_out + 2 * i));
    }
    if (live && len_out) len_out[i] = c;
}

// [a, a + bytes) and [b, b + bytes) share a byte (null: no)
inline bool ranges_overlap(const void* a, const void* b, int64_t bytes) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

}  // namespace

// DynamicsModel.get_state on fp32 observation rows (dynamics.py:190-232): the
// state rcbf_obs_safe_action forms in-kernel (state_from_obs32), one row per thread
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_state_from_obs(int64_t B, const float* __restrict__ obs,
                                                           float* __restrict__ state) {
    using D = Dims<MODE, 1>;
    const int64_t i = env_index();
    if (i >= B) return;
    float o[D::NO], s32[D::NS];
#pragma unroll
    for (int k = 0; k < D::NO; ++k) o[k] = obs[i * D::NO + k];
    state_from_obs32<MODE>(o, s32);
#pragma unroll
    for (int k = 0; k < D::NS; ++k) state[i * D::NS + k] = s32[k];
}

extern "C" {

int rcbf_model_step(const rcbf_params* prm, int64_t B, const double* obs, const double* act, const double* t,
                    const float* mean, const float* stdv, const double* z, uint64_t seed, uint64_t counter,
                    double* next_obs, double* reward, double* mask, double* next_t, hipStream_t stream) {
    if (int e = check_prm(prm)) return e;
    if (B < 0) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!obs || !act || !next_obs || !reward || !mask) return RCBF_E_NULL;
    if (prm->mode == RCBF_MODE_SIMULATED_CARS && !t) return RCBF_E_NULL;  // cars dynamics need t
    dim3 g(grid_for(B)), b(kBlock);
    if (prm->mode == RCBF_MODE_SIMULATED_CARS)
        hipLaunchKernelGGL((k_model_step<RCBF_MODE_SIMULATED_CARS>), g, b, 0, stream, *prm, B, obs, act, t, mean, stdv,
                           z, seed, counter, next_obs, reward, mask, next_t);
    else
        hipLaunchKernelGGL((k_model_step<RCBF_MODE_UNICYCLE>), g, b, 0, stream, *prm, B, obs, act, t, mean, stdv, z,
                           seed, counter, next_obs, reward, mask, next_t);
    return launch_status();
}

int rcbf_predict_next_state(const rcbf_params* prm, int64_t B, const double* x, const double* act, const double* t,
                            const float* mean, const float* stdv, int32_t use_gps, double* next_x, double* std_out,
                            double* next_t, hipStream_t stream) {
    if (int e = check_prm(prm)) return e;
    if (B < 0) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!x || !act || !next_x || !std_out) return RCBF_E_NULL;
    if (prm->mode == RCBF_MODE_SIMULATED_CARS && !t) return RCBF_E_NULL;  // cars dynamics need t
    if (next_t && !t) return RCBF_E_NULL;
    dim3 g(grid_for(B)), b(kBlock);
    if (prm->mode == RCBF_MODE_SIMULATED_CARS)
        hipLaunchKernelGGL((k_predict_next_state<RCBF_MODE_SIMULATED_CARS>), g, b, 0, stream, B, x, act, t, mean,
                           stdv, (int)use_gps, next_x, std_out, next_t);
    else
        hipLaunchKernelGGL((k_predict_next_state<RCBF_MODE_UNICYCLE>), g, b, 0, stream, B, x, act, t, mean, stdv,
                           (int)use_gps, next_x, std_out, next_t);
    return launch_status();
}

int rcbf_state_from_obs(const rcbf_params* prm, int64_t B, const float* obs, float* state_out, hipStream_t stream) {
    if (int e = check_prm(prm)) return e;
    if (B < 0) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!obs || !state_out) return RCBF_E_NULL;
    if (prm->mode == RCBF_MODE_SIMULATED_CARS)
        hipLaunchKernelGGL((k_state_from_obs<RCBF_MODE_SIMULATED_CARS>), dim3(grid_for(B)), dim3(kBlock), 0, stream, B,
                           obs, state_out);
    else
        hipLaunchKernelGGL((k_state_from_obs<RCBF_MODE_UNICYCLE>), dim3(grid_for(B)), dim3(kBlock), 0, stream, B, obs,
                           state_out);
    return launch_status();
}

int rcbf_ring_scatter_f64(double* ring, int64_t cap, int64_t W, int64_t pos, const double* src, int64_t n,
                          hipStream_t stream) {
    if (cap < 1 || W < 1 || n < 0 || pos < 0 || n > cap) return RCBF_E_BAD_SHAPE;
    if (n == 0) return 0;
    if (!ring || !src) return RCBF_E_NULL;
    hipLaunchKernelGGL(k_ring_scatter, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, stream, ring, cap, W,
                       pos % cap, src, n);
    return launch_status();
}

int rcbf_traj_pack_replay_f64(double* ring, int64_t capacity, int64_t position, int64_t B, int32_t K, int64_t P,
                              int32_t n_o, int32_t n_u, const float* obs0, const int32_t* step0, const float* obs,
                              const float* term_obs, const float* u, const float* reward, const uint8_t* done,
                              int32_t max_episode_steps, double dt, int32_t auto_reset, hipStream_t stream) {
    using DC = Dims<RCBF_MODE_SIMULATED_CARS, 1>;
    using DU = Dims<RCBF_MODE_UNICYCLE, 1>;
    const bool cars = n_o == DC::NO && n_u == DC::NU;
    if (!cars && !(n_o == DU::NO && n_u == DU::NU)) return RCBF_E_BAD_SHAPE;
    if (B < 0 || K <= 0 || P < B || capacity <= 0 || position < 0 || position >= capacity) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!ring || !obs0 || !step0 || !obs || !u || !reward || !done) return RCBF_E_NULL;
    // cars rows are read as 8-byte pairs
    if (cars && ((((uintptr_t)obs0) | ((uintptr_t)obs) | ((uintptr_t)term_obs)) & 7)) return RCBF_E_BAD_SHAPE;
    if ((((uintptr_t)ring) & 7) || B > INT32_MAX) return RCBF_E_BAD_SHAPE;
    const int64_t n = (int64_t)K * B;
    const int64_t skip = n > capacity ? n - capacity : 0;
    const int64_t waves = (B + 63) / 64;
    const int chunk = traj_steps_per_workgroup(waves, K);
    const dim3 g((unsigned)waves, (unsigned)((K + chunk - 1) / chunk)), b(64);
    if (cars)
        hipLaunchKernelGGL((k_traj_pack_replay<DC::NO, DC::NU>), g, b, 0, stream, ring, capacity, position, skip, B,
                           (int)K, P, obs0, step0, obs, term_obs, u, reward, done, (int)max_episode_steps, dt,
                           (int)auto_reset, chunk);
    else
        hipLaunchKernelGGL((k_traj_pack_replay<DU::NO, DU::NU>), g, b, 0, stream, ring, capacity, position, skip, B,
                           (int)K, P, obs0, step0, obs, term_obs, u, reward, done, (int)max_episode_steps, dt,
                           (int)auto_reset, chunk);
    return launch_status();
}

int64_t rcbf_traj_pack_gp_scratch_bytes(int64_t B, int32_t K) {
    if (B < 0 || K <= 0) return 0;
    return 8 * (((B + 63) / 64) * (int64_t)K + 1);  // a count per (step, wave), and the total
}

int rcbf_traj_pack_gp_f64(double* state_out, double* dist_out, int64_t* count_out, void* scratch, int64_t B,
                          int32_t K, int64_t P, int32_t n_o, int32_t n_u, const float* obs0, const int32_t* step0,
                          const float* obs, const float* term_obs, const float* u, const uint8_t* done, double dt,
                          int32_t auto_reset, int32_t every, int64_t keep_last, hipStream_t stream) {
    using DC = Dims<RCBF_MODE_SIMULATED_CARS, 1>;
    using DU = Dims<RCBF_MODE_UNICYCLE, 1>;
    const bool cars = n_o == DC::NO && n_u == DC::NU;
    if (!cars && !(n_o == DU::NO && n_u == DU::NU)) return RCBF_E_BAD_SHAPE;
    if (B < 0 || K <= 0 || P < B || every < 1 || keep_last < 1) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!state_out || !dist_out || !count_out || !scratch || !obs0 || !step0 || !obs || !u || !done)
        return RCBF_E_NULL;
    // a reset row as x' would be a garbage disturbance: no terminal rows, no auto-reset packing
    if (auto_reset && !term_obs) return RCBF_E_NULL;
    // cars rows are read as 8-byte pairs
    if (cars && ((((uintptr_t)obs0) | ((uintptr_t)obs) | ((uintptr_t)term_obs)) & 7)) return RCBF_E_BAD_SHAPE;
    if (((((uintptr_t)state_out) | ((uintptr_t)dist_out) | ((uintptr_t)count_out) | ((uintptr_t)scratch)) & 7) ||
        B > INT32_MAX)
        return RCBF_E_BAD_SHAPE;
    const int64_t waves = (B + 63) / 64;
    const int chunk = traj_steps_per_workgroup(waves, K);
    const dim3 g((unsigned)waves, (unsigned)((K + chunk - 1) / chunk)), b(64);
    int64_t* const offs = static_cast<int64_t*>(scratch);
    hipLaunchKernelGGL(k_traj_gp_count, g, b, 0, stream, offs, B, (int)K, P, step0, done, (int)auto_reset, (int)every,
                       chunk);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(k_traj_gp_scan, dim3(1), dim3(1024), 0, stream, offs, waves * K, keep_last, count_out);
    if (int e = launch_status()) return e;
    if (cars)
        hipLaunchKernelGGL((k_traj_pack_gp<RCBF_MODE_SIMULATED_CARS>), g, b, 0, stream, state_out, dist_out, offs,
                           keep_last, B, (int)K, P, obs0, step0, obs, term_obs, u, done, dt, (int)auto_reset,
                           (int)every, chunk);
    else
        hipLaunchKernelGGL((k_traj_pack_gp<RCBF_MODE_UNICYCLE>), g, b, 0, stream, state_out, dist_out, offs,
                           keep_last, B, (int)K, P, obs0, step0, obs, term_obs, u, done, dt, (int)auto_reset,
                           (int)every, chunk);
    return launch_status();
}

int64_t rcbf_traj_episode_stats_scratch_bytes(int64_t B, int32_t K) {
    if (B < 0 || K <= 0) return 0;
    return 8 * (((B + 63) / 64) * (int64_t)K + 1);  // a count per (step, wave), and the total
}

int rcbf_traj_episode_stats_f64(int32_t* ep_env, int32_t* ep_step, int32_t* ep_len, double* ep_return,
                                double* ep_cost, int64_t* count_out, void* scratch, int64_t B, int32_t K, int64_t P,
                                const float* reward, const float* cost, const uint8_t* done, const double* carry_in,
                                const int32_t* len_in, double* carry_out, int32_t* len_out, int32_t auto_reset,
                                int64_t max_rows, hipStream_t stream) {
    if (B < 0 || K <= 0 || P < B || max_rows < 0 || B > INT32_MAX) return RCBF_E_BAD_SHAPE;
    if (B == 0) return 0;
    if (!reward || !done || !count_out || !scratch) return RCBF_E_NULL;
    if (max_rows > 0 && (!ep_env || !ep_step || !ep_len || !ep_return || !ep_cost)) return RCBF_E_NULL;
    auto at = [](const void* p) { return (uintptr_t)p; };
    if ((at(carry_in) | at(carry_out)) & 15) return RCBF_E_BAD_SHAPE;  // a lane's (R, C) is one 16-byte access
    if ((at(ep_return) | at(ep_cost) | at(count_out) | at(scratch)) & 7) return RCBF_E_BAD_SHAPE;
    if ((at(ep_env) | at(ep_step) | at(ep_len) | at(reward) | at(cost) | at(len_in) | at(len_out)) & 3)
        return RCBF_E_BAD_SHAPE;
    // in and out are separate arrays: a lane reads its carry where another call's lane may be writing its own
    if (ranges_overlap(carry_in, carry_out, 16 * B) || ranges_overlap(len_in, len_out, 4 * B)) return RCBF_E_BAD_SHAPE;
    const int64_t waves = (B + 63) / 64;
    const int chunk = traj_steps_per_workgroup(waves, K);
    int64_t* const offs = static_cast<int64_t*>(scratch);
    hipLaunchKernelGGL(k_traj_ep_count, dim3((unsigned)waves, (unsigned)((K + chunk - 1) / chunk)), dim3(64), 0, stream,
                       offs, B, (int)K, P, done, (int)auto_reset, chunk);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(k_traj_gp_scan, dim3(1), dim3(1024), 0, stream, offs, waves * K, max_rows, count_out);
    if (int e = launch_status()) return e;
    if (max_rows == 0 && !carry_out && !len_out) return 0;  // the count-only call: the pack pass would write nothing
    // the pack pass: a lane walks all K steps of its env (the sums are serial); no split over the steps
    const dim3 g((unsigned)waves), b(64);
    if (cost)
        hipLaunchKernelGGL((k_traj_ep_pack<true>), g, b, 0, stream, ep_env, ep_step, ep_len, ep_return, ep_cost, offs,
                           max_rows, B, (int)K, P, reward, cost, done, carry_in, len_in, carry_out, len_out,
                           (int)auto_reset);
    else
        hipLaunchKernelGGL((k_traj_ep_pack<false>), g, b, 0, stream, ep_env, ep_step, ep_len, ep_return, ep_cost, offs,
                           max_rows, B, (int)K, P, reward, cost, done, carry_in, len_in, carry_out, len_out,
                           (int)auto_reset);
    return launch_status();
}

int rcbf_gather_rows_f64(double* dst, const double* ring, int64_t W, const int64_t* idx, int64_t n,
                         hipStream_t stream) {
    if (W < 1 || n < 0) return RCBF_E_BAD_SHAPE;
    if (n == 0) return 0;
    if (!dst || !ring || !idx) return RCBF_E_NULL;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, stream, dst, ring, W, idx,
                       n);
    return launch_status();
}

}  // extern "C"
