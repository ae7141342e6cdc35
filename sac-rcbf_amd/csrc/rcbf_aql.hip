// rcbf_aql.hip -- the fused safe step dispatched as raw AQL packets on a
// user-mode HSA queue owned by the library (host code only; no kernels here).
//
// Why: a step of the hot path is ~3.6 us of GPU time, and the HIP launch path
// costs more than that around a short sequence of them: hipGraphLaunch spends
// ~16-25 us of host time on a 20-node graph and the first kernel starts ~17 us
// after the event recorded before it (profiles/README.md, r02 narrative);
// hipLaunchKernel costs ~5 us of host time per launch.  The driver's 20-step
// bench line therefore spends ~30 % of its wall time outside the kernels.
//
// What: the kernels are the SAME machine code HIP launches -- the gfx950 code
// object embedded in rcbf_env.o, unbundled at build time into
// librcbf_steps.co next to librcbf_hip.so -- loaded once into an HSA
// executable.  A "plan" is the AQL analogue of an instantiated hipGraph: the
// kernel-argument blocks of K steps written once into device memory and the K
// dispatch packets pre-built on the host.  Running a plan copies the K packets
// into the queue's ring (60 B each + an atomic header store), rings the
// doorbell once and waits on the last packet's completion signal, so the
// host-side cost of K dispatches is ~1 us and the packet processor starts the
// first kernel as soon as it reads the packet.  Every packet has the barrier
// bit: step j + 1 starts after step j has completed, exactly like K launches
// on one in-order stream.  Memory scopes: the last packet releases at system
// scope (the host reads the completion signal; HIP work after the call sees
// the results), the packets between
// acquire and release at agent scope, which on gfx950 writes the XCD L2s back
// and invalidates them between steps as HIP's in-order stream does.  The first
// packet acquires at agent scope: every input of the step is device memory
// written by device work or copies that completed before the run (a system-
// scope acquire there cost the first step ~3 us: profiles/r06/aql_fences_r06e.json).
//
// The fused form (r07).  A plan's actions are all known before it starts, and
// env i at step j + 1 reads only what env i wrote at step j, so a plan of
// K > 1 steps is ONE dispatch of rcbf::k_safe_steps (one per 4 096 steps) in
// which each lane runs its env's steps back to back, every step storing
// everything a step stores: the K - 1 fences and state re-loads between the
// dispatches go away, memory ends up as K dispatches leave it.  When it
// applies is decided in rcbf_aql_safe_step_plan; everything said above about
// K packets describes the per-step form, which remains for K = 1, the other
// solvers, span / per-dispatch-profiled / study plans, RCBF_AQL_PER_STEP and
// action buffers that alias an output.
//
// The closed-loop form (rcbf_aql_closed_loop_plan).  When the policy acts between the steps, step j's action
// is not known before the run: it is what the actor computes from the observation step j - 1 left.  Such a
// plan is 2K packets, a policy packet (rcbf::k_policy_step, from librcbf_policy.co) before every step packet,
// each with the barrier bit and the per-step form's fences: the policy writes one (B, n_u) action buffer, the
// step reads it and leaves the observation the next policy packet reads.  Per-step by nature, it never takes
// the fused form; with RCBF_TRAJ_TERM_OBS its step packets are one-step dispatches of k_safe_steps_term.
//
// Reference interface this serves: env.step() of the batched env inside the
// SAC loop (main.py:93-95, sac_cbf.py:218-238) -- a synchronous call, like a
// gym step: rcbf_aql_run returns when the K steps have completed.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <dlfcn.h>
#include <immintrin.h>
#include <time.h>

#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rcbf_hip.h"
#include "rcbf_policy_step.hpp"  // PolicyStepArgs, the policy packet of a closed-loop plan
#include "rcbf_safe_step.hpp"  // SafeStepsArgs (the templates in it are not instantiated here)

namespace {

using namespace rcbf;

// Kernel-argument block of rcbf::k_safe_step (rcbf_safe_step.hpp), in the
// order and at the offsets of its parameter list (the AMDGPU kernarg ABI:
// every argument at its natural alignment, by-value structs included).  The
// kernel reads no hidden arguments (its code-object metadata lists none and
// its kernarg_segment_size is 408), which rcbf_aql_open checks against the
// loaded code object before any dispatch; tests/test_abi_cpu.py checks the
// offsets against the metadata of librcbf_steps.co on the CPU.
struct SafeStepArgs {
    int64_t B;
    double* x;
    double* aux;
    int32_t* step;
    const float* u_rl;
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
    unsigned long long* stamp_buf;
};
static_assert(offsetof(SafeStepArgs, auto_reset) == 128, "kernarg layout");
static_assert(offsetof(SafeStepArgs, seed) == 136, "kernarg layout");
static_assert(offsetof(SafeStepArgs, prm) == 152, "kernarg layout");
static_assert(offsetof(SafeStepArgs, prior_cols) == 392, "kernarg layout");
static_assert(offsetof(SafeStepArgs, stamp_buf) == 400, "kernarg layout");
static_assert(sizeof(SafeStepArgs) == RCBF_AQL_SAFE_STEP_KERNARG_BYTES, "kernarg layout");
// the fused form's kernel (rcbf::k_safe_steps) takes rcbf::SafeStepsArgs, defined next to it
static_assert(sizeof(SafeStepsArgs) == RCBF_AQL_SAFE_STEPS_KERNARG_BYTES, "kernarg layout");
// ... and its trajectory form (rcbf::k_safe_steps_traj) rcbf::SafeStepsTrajArgs
static_assert(sizeof(SafeStepsTrajArgs) == RCBF_AQL_SAFE_STEPS_TRAJ_KERNARG_BYTES, "kernarg layout");
// ... and the form that keeps the terminal observation (rcbf::k_safe_steps_term) rcbf::SafeStepsTermArgs
static_assert(sizeof(SafeStepsTermArgs) == RCBF_AQL_SAFE_STEPS_TERM_KERNARG_BYTES, "kernarg layout");

struct KernelInfo {
    std::string name;  // mangled symbol without ".kd"
    uint64_t object = 0;
    uint32_t kernarg_bytes = 0, group_bytes = 0, private_bytes = 0;
};

constexpr uint32_t kQueueSize = 4096;  // packets (power of two); a plan longer than this is fed in chunks
constexpr size_t kArgStride = 512;     // bytes per step's kernarg block (>= 432, 64-B multiple)
static_assert(sizeof(SafeStepsTermArgs) <= kArgStride, "kernarg block");
constexpr int32_t kTrajAll = RCBF_TRAJ_OBS | RCBF_TRAJ_U | RCBF_TRAJ_REWARD | RCBF_TRAJ_COST | RCBF_TRAJ_DONE |
                             RCBF_TRAJ_GOAL_MET | RCBF_TRAJ_STATUS;
constexpr int32_t kFusedChunk = (int32_t)kQueueSize;  // most steps one fused dispatch runs: a bounded kernel

uint64_t now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

}  // namespace

struct rcbf_aql {
    int device = -1;
    hsa_agent_t agent{};
    hsa_queue_t* queue = nullptr;
    hsa_code_object_reader_t reader{};
    hsa_code_object_reader_t reader_traj{};  // librcbf_steps_traj.co (the k_safe_steps_traj kernels), if there
    hsa_executable_t exe{};
    hsa_executable_t exe_traj{};  // its own executable: no symbol of one code object can meet one of the other
    hsa_code_object_reader_t reader_term{};  // librcbf_steps_term.co (the k_safe_steps_term kernels), if there
    hsa_executable_t exe_term{};
    bool have_reader = false, have_reader_traj = false, have_exe = false, have_exe_traj = false, hsa_up = false;
    bool have_reader_term = false, have_exe_term = false;
    hsa_code_object_reader_t reader_policy{};  // librcbf_policy.co (the k_policy_step kernels), if there
    hsa_executable_t exe_policy{};
    bool have_reader_policy = false, have_exe_policy = false;
    hsa_code_object_reader_t reader_fast{};  // librcbf_steps_fast.co (the k_safe_steps_fast kernels), if there
    hsa_executable_t exe_fast{};
    bool have_reader_fast = false, have_exe_fast = false;
    std::vector<char> code, code_traj, code_term, code_policy, code_fast;
    std::vector<KernelInfo> kernels;
    std::atomic<int> queue_error{0};
    int profiling = 0;
    bool fused = false;  // the code object has the k_safe_steps kernels (the fused plan form)
    bool traj = false;   // ... and the k_safe_steps_traj kernels (the fused form of a trajectory plan)
    bool term = false;   // ... and the k_safe_steps_term kernels (trajectory plans with RCBF_TRAJ_TERM_OBS)
    bool fast = false;   // ... and the three k_safe_steps_fast kernels (the cars fused plan's straight-line loop)
    bool policy = false;  // the four k_policy_step kernels were found, each taking PolicyStepArgs (closed-loop plans)
};

struct rcbf_aql_plan {
    rcbf_aql* q = nullptr;
    int device = -1;  // the queue's HIP device (rcbf_aql_plan_free does not read q: a plan may outlive it)
    int32_t K = 0;                                  // steps per run
    void* kernargs = nullptr;                       // one kArgStride block per packet (+ the fused form's u_RL table)
    std::vector<hsa_kernel_dispatch_packet_t> pkt;  // pre-built packets (header written last, atomically)
    std::vector<hsa_signal_t> sig;                  // completion signals: one per packet (profiled), first and
                                                    // last (ends; one if they are the same packet), or one
    int profiled = 0;
    int form = RCBF_AQL_FORM_PER_STEP;  // RCBF_AQL_FORM_*: the kernel its step packets dispatch
};

namespace {

void queue_error_cb(hsa_status_t status, hsa_queue_t*, void* data) {
    auto* q = static_cast<rcbf_aql*>(data);
    q->queue_error.store((int)status);
}

struct AgentSearch {
    uint32_t bdf;
    uint32_t domain;
    hsa_agent_t found{};
    bool ok = false;
};

hsa_status_t find_agent(hsa_agent_t a, void* data) {
    auto* s = static_cast<AgentSearch*>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU)
        return HSA_STATUS_SUCCESS;
    uint32_t bdf = 0, dom = 0;
    if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS)
        return HSA_STATUS_SUCCESS;
    hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
    // BDFID = bus << 8 | device << 3 | function
    if ((bdf >> 3) == (s->bdf >> 3) && dom == s->domain) {
        s->found = a;
        s->ok = true;
        return HSA_STATUS_INFO_BREAK;
    }
    return HSA_STATUS_SUCCESS;
}

hsa_status_t collect_kernel(hsa_executable_t, hsa_agent_t, hsa_executable_symbol_t sym, void* data) {
    auto* q = static_cast<rcbf_aql*>(data);
    hsa_symbol_kind_t kind;
    if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_TYPE, &kind) != HSA_STATUS_SUCCESS ||
        kind != HSA_SYMBOL_KIND_KERNEL)
        return HSA_STATUS_SUCCESS;
    uint32_t len = 0;
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME_LENGTH, &len);
    std::string name(len, '\0');
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME, name.data());
    if (name.size() > 3 && name.compare(name.size() - 3, 3, ".kd") == 0) name.resize(name.size() - 3);
    KernelInfo k;
    k.name = name;
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object);
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k.kernarg_bytes);
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k.group_bytes);
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k.private_bytes);
    q->kernels.push_back(std::move(k));
    return HSA_STATUS_SUCCESS;
}

// Itanium mangling of rcbf::k_safe_step<SOLVER, MODE, K, false, BS, SPAN>'s
// name and template arguments; the parameter list that follows is the one
// SafeStepArgs mirrors (checked by size at open and by the CPU test).
std::string safe_step_prefix(int solver, int mode, int k, int bs, bool span) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf11k_safe_stepILi%dELi%dELi%dELb0ELi%dELb%dEEEv", solver, mode, k, bs,
             span ? 1 : 0);
    return buf;
}

// ... and of rcbf::k_safe_steps<MODE, K, BS> (SafeStepsArgs)
std::string safe_steps_prefix(int mode, int k, int bs) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf12k_safe_stepsILi%dELi%dELi%dEEEv", mode, k, bs);
    return buf;
}

// ... and of rcbf::k_safe_steps_traj<MODE, K, BS> (SafeStepsTrajArgs)
std::string safe_steps_traj_prefix(int mode, int k, int bs) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf17k_safe_steps_trajILi%dELi%dELi%dEEEv", mode, k, bs);
    return buf;
}

// ... and of rcbf::k_safe_steps_term<MODE, K, BS> (SafeStepsTermArgs)
std::string safe_steps_term_prefix(int mode, int k, int bs) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf17k_safe_steps_termILi%dELi%dELi%dEEEv", mode, k, bs);
    return buf;
}

// ... and of rcbf::k_safe_steps_fast<BS> (SafeStepsArgs)
std::string safe_steps_fast_prefix(int bs) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf17k_safe_steps_fastILi%dEEEv", bs);
    return buf;
}

// ... and of rcbf::k_policy_step<SAMPLE, NRB> (PolicyStepArgs)
std::string policy_step_prefix(bool sample, int nrb) {
    char buf[128];
    snprintf(buf, sizeof buf, "_ZN4rcbf13k_policy_stepILb%dELi%dEEEv", sample ? 1 : 0, nrb);
    return buf;
}

bool read_optional_code_object(const std::string& tpath, std::vector<char>& code);

// The optional code object NAME<suffix>.co beside NAME.co, read whole into `code` (left empty when the file is
// not there).  false: there, but unreadable -- an error, not a quiet fall back.
bool read_side_code_object(const std::string& path, const char* suffix, std::vector<char>& code) {
    if (path.size() <= 3 || path.compare(path.size() - 3, 3, ".co") != 0) return true;
    return read_optional_code_object(path.substr(0, path.size() - 3) + suffix + ".co", code);
}

// The policy kernels' code object beside NAME.co: DIR/librcbf_policy.co for DIR/librcbf_steps.co (the build's
// names), NAME_policy.co for any other name.
std::string policy_code_object_path(const std::string& path) {
    static const char kSteps[] = "librcbf_steps.co";
    const size_t n = sizeof kSteps - 1;
    if (path.size() >= n && path.compare(path.size() - n, n, kSteps) == 0 &&
        (path.size() == n || path[path.size() - n - 1] == '/'))
        return path.substr(0, path.size() - n) + "librcbf_policy.co";
    if (path.size() <= 3 || path.compare(path.size() - 3, 3, ".co") != 0) return std::string();
    return path.substr(0, path.size() - 3) + "_policy.co";
}

bool read_optional_code_object(const std::string& tpath, std::vector<char>& code) {
    if (tpath.empty()) return true;
    FILE* tf = fopen(tpath.c_str(), "rb");
    if (!tf) return true;
    fseek(tf, 0, SEEK_END);
    const long tn = ftell(tf);
    fseek(tf, 0, SEEK_SET);
    code.resize(tn > 0 ? (size_t)tn : 0);
    const bool ok = tn > 0 && fread(code.data(), 1, (size_t)tn, tf) == (size_t)tn;
    fclose(tf);
    return ok;
}

// p moved on by `rows` rows of `row_bytes` bytes (64-bit arithmetic); a null pointer stays null
template <typename T>
T* rows_on(T* p, int64_t rows, int64_t row_bytes) {
    return p ? reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(p) + rows * row_bytes) : nullptr;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// What the argument block of every step kernel (SafeStepArgs, SafeStepsArgs) takes from the plan's arguments; the
// action source and the form's own fields are the caller's.
struct StepIo {
    const rcbf_params* prm;
    int64_t B;
    double* x;
    double* aux;
    int32_t* step;
    uint32_t* episode;
    const float* mu;
    const float* sigma;
    int32_t prior_cols;
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
    int64_t env_offset;
    // bytes of one row of each output's (K, P, w) array; 0: not recorded (written in place)
    int64_t row_obs, row_u, row_rew, row_cost, row_done, row_goal, row_stat;

    // a zeroed block with the shared fields set, each recorded output at row r0 of its array
    template <typename Args>
    void fill(Args& a, int64_t r0) const {
        std::memset(&a, 0, sizeof a);
        a.B = B;
        a.x = x;
        a.aux = aux;
        a.step = step;
        a.episode = episode;
        a.mu = mu;
        a.sigma = sigma;
        a.obs_out = rows_on(obs_out, r0, row_obs);
        a.u_out = rows_on(u_out, r0, row_u);
        a.reward = rows_on(reward, r0, row_rew);
        a.cost = rows_on(cost, r0, row_cost);
        a.done = rows_on(done, r0, row_done);
        a.goal_met = rows_on(goal_met, r0, row_goal);
        a.status_out = rows_on(status_out, r0, row_stat);
        a.fail_flag = fail_flag;
        a.auto_reset = auto_reset;
        a.seed = seed;
        a.off = env_offset;
        a.prm = *prm;
        a.prior_cols = prior_cols ? 1 : 0;
    }
};

const KernelInfo* find_kernel(const rcbf_aql* q, const std::string& prefix) {
    const KernelInfo* hit = nullptr;
    for (const auto& k : q->kernels)
        if (k.name.compare(0, prefix.size(), prefix) == 0) {
            if (hit) return nullptr;  // ambiguous
            hit = &k;
        }
    return hit;
}

int hsa_rc(hsa_status_t s) { return s == HSA_STATUS_SUCCESS ? 0 : RCBF_E_HSA; }

// Current HIP device set to `dev` for the scope (kernarg copies, CU count).
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

void destroy(rcbf_aql* q) {
    if (!q) return;
    if (q->queue) hsa_queue_destroy(q->queue);
    if (q->have_exe) hsa_executable_destroy(q->exe);
    if (q->have_exe_traj) hsa_executable_destroy(q->exe_traj);
    if (q->have_exe_term) hsa_executable_destroy(q->exe_term);
    if (q->have_exe_policy) hsa_executable_destroy(q->exe_policy);
    if (q->have_exe_fast) hsa_executable_destroy(q->exe_fast);
    if (q->have_reader_fast) hsa_code_object_reader_destroy(q->reader_fast);
    if (q->have_reader_policy) hsa_code_object_reader_destroy(q->reader_policy);
    if (q->have_reader) hsa_code_object_reader_destroy(q->reader);
    if (q->have_reader_traj) hsa_code_object_reader_destroy(q->reader_traj);
    if (q->have_reader_term) hsa_code_object_reader_destroy(q->reader_term);
    if (q->hsa_up) hsa_shut_down();
    delete q;
}

}  // namespace

extern "C" {

int rcbf_aql_open(int32_t device, const char* code_object_path, int32_t flags, rcbf_aql** out) {
    if (!out) return RCBF_E_NULL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RCBF_E_BAD_SHAPE;
    std::string path;
    if (code_object_path && *code_object_path) {
        path = code_object_path;
    } else {  // librcbf_steps.co next to this library
        Dl_info info;
        if (!dladdr((void*)&rcbf_aql_open, &info) || !info.dli_fname) return RCBF_E_NULL;
        path = info.dli_fname;
        const size_t slash = path.rfind('/');
        path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/librcbf_steps.co";
    }
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return RCBF_E_NULL;
    auto* q = new rcbf_aql();
    q->device = device;
    q->profiling = (flags & RCBF_AQL_PROFILE) ? 1 : 0;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    q->code.resize(n > 0 ? (size_t)n : 0);
    const bool read_ok = n > 0 && fread(q->code.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!read_ok) {
        delete q;
        return RCBF_E_BAD_SHAPE;
    }
    // the trajectory plans' kernels: NAME_traj.co beside NAME.co.  Without it the queue opens as before and
    // trajectory plans take the per-step form.
    if (!read_side_code_object(path, "_traj", q->code_traj)) {
        delete q;
        return RCBF_E_BAD_SHAPE;
    }
    // ... and NAME_term.co, the kernels of the plans that keep the terminal observation: without it those
    // plans are refused (they have no per-step form) and everything else works as before
    if (!read_side_code_object(path, "_term", q->code_term)) {
        delete q;
        return RCBF_E_BAD_SHAPE;
    }
    // ... and the policy kernels of the closed-loop plans (librcbf_policy.co): without it those plans are refused
    if (!read_optional_code_object(policy_code_object_path(path), q->code_policy)) {
        delete q;
        return RCBF_E_BAD_SHAPE;
    }
    // ... and NAME_fast.co, the cars fused plan's straight-line loop: without it those plans take k_safe_steps
    if (!read_side_code_object(path, "_fast", q->code_fast)) {
        delete q;
        return RCBF_E_BAD_SHAPE;
    }
    int rc = hsa_rc(hsa_init());
    if (rc) {
        delete q;
        return rc;
    }
    q->hsa_up = true;
    // the HSA agent of HIP device `device`, matched by PCI location (HIP's device
    // ordinals follow HIP_VISIBLE_DEVICES, HSA's agent list does not)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        destroy(q);
        return RCBF_E_HSA;
    }
    AgentSearch s{(uint32_t)((prop.pciBusID << 8) | (prop.pciDeviceID << 3)), (uint32_t)prop.pciDomainID};
    hsa_iterate_agents(find_agent, &s);
    if (!s.ok) {
        destroy(q);
        return RCBF_E_HSA;
    }
    q->agent = s.found;
    rc = hsa_rc(hsa_code_object_reader_create_from_memory(q->code.data(), q->code.size(), &q->reader));
    if (!rc) q->have_reader = true;
    if (!rc)
        rc = hsa_rc(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                              &q->exe));
    if (!rc) q->have_exe = true;
    if (!rc) rc = hsa_rc(hsa_executable_load_agent_code_object(q->exe, q->agent, q->reader, nullptr, nullptr));
    if (!rc) rc = hsa_rc(hsa_executable_freeze(q->exe, nullptr));
    if (!rc) rc = hsa_rc(hsa_executable_iterate_agent_symbols(q->exe, q->agent, collect_kernel, q));
    if (!rc && !q->code_traj.empty()) {
        rc = hsa_rc(
            hsa_code_object_reader_create_from_memory(q->code_traj.data(), q->code_traj.size(), &q->reader_traj));
        if (!rc) q->have_reader_traj = true;
        if (!rc)
            rc = hsa_rc(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                                  &q->exe_traj));
        if (!rc) q->have_exe_traj = true;
        if (!rc)
            rc = hsa_rc(
                hsa_executable_load_agent_code_object(q->exe_traj, q->agent, q->reader_traj, nullptr, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_freeze(q->exe_traj, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_iterate_agent_symbols(q->exe_traj, q->agent, collect_kernel, q));
    }
    if (!rc && !q->code_term.empty()) {
        rc = hsa_rc(
            hsa_code_object_reader_create_from_memory(q->code_term.data(), q->code_term.size(), &q->reader_term));
        if (!rc) q->have_reader_term = true;
        if (!rc)
            rc = hsa_rc(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                                  &q->exe_term));
        if (!rc) q->have_exe_term = true;
        if (!rc)
            rc = hsa_rc(
                hsa_executable_load_agent_code_object(q->exe_term, q->agent, q->reader_term, nullptr, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_freeze(q->exe_term, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_iterate_agent_symbols(q->exe_term, q->agent, collect_kernel, q));
    }
    if (!rc && !q->code_policy.empty()) {
        rc = hsa_rc(hsa_code_object_reader_create_from_memory(q->code_policy.data(), q->code_policy.size(),
                                                              &q->reader_policy));
        if (!rc) q->have_reader_policy = true;
        if (!rc)
            rc = hsa_rc(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                                  &q->exe_policy));
        if (!rc) q->have_exe_policy = true;
        if (!rc)
            rc = hsa_rc(
                hsa_executable_load_agent_code_object(q->exe_policy, q->agent, q->reader_policy, nullptr, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_freeze(q->exe_policy, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_iterate_agent_symbols(q->exe_policy, q->agent, collect_kernel, q));
    }
    if (!rc && !q->code_fast.empty()) {
        rc = hsa_rc(
            hsa_code_object_reader_create_from_memory(q->code_fast.data(), q->code_fast.size(), &q->reader_fast));
        if (!rc) q->have_reader_fast = true;
        if (!rc)
            rc = hsa_rc(hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
                                                  &q->exe_fast));
        if (!rc) q->have_exe_fast = true;
        if (!rc)
            rc = hsa_rc(
                hsa_executable_load_agent_code_object(q->exe_fast, q->agent, q->reader_fast, nullptr, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_freeze(q->exe_fast, nullptr));
        if (!rc) rc = hsa_rc(hsa_executable_iterate_agent_symbols(q->exe_fast, q->agent, collect_kernel, q));
    }
    // every k_safe_step instantiation in the code object must take exactly the
    // argument block SafeStepArgs describes
    // ... and every k_safe_steps instantiation SafeStepsArgs; a code object without them still opens, and
    // its plans take the per-step form; likewise k_safe_steps_traj and SafeStepsTrajArgs
    int n_steps = 0, n_fused = 0, n_traj = 0, n_term = 0;
    for (const auto& k : q->kernels) {
        if (k.name.compare(0, 21, "_ZN4rcbf11k_safe_step") == 0) {
            ++n_steps;
            if (k.kernarg_bytes != sizeof(SafeStepArgs) || k.private_bytes != 0) rc = RCBF_E_BAD_SHAPE;
        } else if (k.name.compare(0, 22, "_ZN4rcbf12k_safe_steps") == 0) {
            ++n_fused;
            if (k.kernarg_bytes != sizeof(SafeStepsArgs) || k.private_bytes != 0) rc = RCBF_E_BAD_SHAPE;
        } else if (k.name.compare(0, 27, "_ZN4rcbf17k_safe_steps_traj") == 0) {
            ++n_traj;
            if (k.kernarg_bytes != sizeof(SafeStepsTrajArgs) || k.private_bytes != 0) rc = RCBF_E_BAD_SHAPE;
        } else if (k.name.compare(0, 27, "_ZN4rcbf17k_safe_steps_term") == 0) {
            ++n_term;
            if (k.kernarg_bytes != sizeof(SafeStepsTermArgs) || k.private_bytes != 0) rc = RCBF_E_BAD_SHAPE;
        }
    }
    if (!rc && n_steps == 0) rc = RCBF_E_BAD_MODE;
    q->fused = n_fused > 0;
    q->traj = n_traj > 0;
    q->term = n_term > 0;
    // the straight-line cars loop, at the three workgroup sizes: all three, each taking SafeStepsArgs and no
    // scratch, or no plan takes it (nothing else is affected)
    int n_fast = 0;
    for (int bs : {64, 128, 256}) {
        const KernelInfo* kp = find_kernel(q, safe_steps_fast_prefix(bs));
        if (kp && kp->kernarg_bytes == sizeof(SafeStepsArgs) && kp->private_bytes == 0) ++n_fast;
    }
    q->fast = n_fast == 3;
    // the closed-loop plans' policy kernels, {mean, sample} x {32-row, 64-row tiles}: all four, each taking
    // PolicyStepArgs and no scratch, or no closed-loop plan is built on this queue (nothing else is affected)
    int n_policy = 0;
    for (int s = 0; s < 2; ++s)
        for (int nrb = 1; nrb <= 2; ++nrb) {
            const KernelInfo* kp = find_kernel(q, policy_step_prefix(s != 0, nrb));
            if (kp && kp->kernarg_bytes == sizeof(PolicyStepArgs) && kp->private_bytes == 0) ++n_policy;
        }
    q->policy = n_policy == 4;
    if (!rc)
        rc = hsa_rc(hsa_queue_create(q->agent, kQueueSize, HSA_QUEUE_TYPE_SINGLE, queue_error_cb, q, UINT32_MAX,
                                     UINT32_MAX, &q->queue));
    if (!rc && q->profiling) rc = hsa_rc(hsa_amd_profiling_set_profiler_enabled(q->queue, 1));
    if (rc) {
        destroy(q);
        return rc;
    }
    *out = q;
    return 0;
}

int rcbf_aql_close(rcbf_aql* q) {
    destroy(q);
    return 0;
}

int rcbf_aql_kernel_count(const rcbf_aql* q) { return q ? (int)q->kernels.size() : RCBF_E_NULL; }

// rcbf_aql_safe_step_plan (traj_mask = 0), rcbf_aql_safe_step_traj_plan (term_obs = nullptr) and
// rcbf_aql_safe_step_term_plan
static int build_safe_step_plan(rcbf_aql* q, const rcbf_params* prm, int64_t B, int32_t K, double* x, double* aux,
                                int32_t* step, uint32_t* episode, const float* const* u_rl_seq, int32_t n_u_rl,
                                const float* mu, const float* sigma, int32_t prior_cols, float* obs_out,
                                float* u_out, float* reward, float* cost, uint8_t* done, uint8_t* goal_met,
                                int32_t* status_out, int32_t* fail_flag, int32_t auto_reset, uint64_t seed,
                                int64_t env_offset, uint64_t* span_out, int32_t flags, int32_t traj_mask,
                                int64_t traj_pitch, float* term_obs, rcbf_aql_plan** out) {
    if (!q || !out) return RCBF_E_NULL;
    *out = nullptr;
    if (int e = check_prm(prm)) return e;
    if (B <= 0 || K <= 0 || n_u_rl <= 0 || B > INT32_MAX) return RCBF_E_BAD_SHAPE;
    if (!u_rl_seq) return RCBF_E_NULL;
    for (int32_t j = 0; j < n_u_rl; ++j)
        if (!u_rl_seq[j]) return RCBF_E_NULL;
    if (!x || !aux || !step || !obs_out || !u_out || !reward || !cost || !done) return RCBF_E_NULL;
    if ((((uintptr_t)obs_out) & 7) || (((uintptr_t)x) & 15)) return RCBF_E_BAD_SHAPE;
    if (prior_cols && prm->mode == RCBF_MODE_SIMULATED_CARS && mu) return RCBF_E_BAD_SHAPE;
    if (span_out && (((uintptr_t)span_out) & 15)) return RCBF_E_BAD_SHAPE;
    if (span_out && prm->solver != RCBF_SOLVER_ACTIVE_SET) return RCBF_E_BAD_MODE;
    // the trajectory contract (rcbf_hip.h)
    // RCBF_TRAJ_TERM_OBS and its pointer come together (rcbf_aql_safe_step_term_plan) or not at all
    const bool term = (traj_mask & RCBF_TRAJ_TERM_OBS) != 0;
    if (term != (term_obs != nullptr)) return RCBF_E_BAD_MODE;
    if (traj_mask & ~(kTrajAll | RCBF_TRAJ_TERM_OBS)) return RCBF_E_BAD_MODE;
    if (traj_mask && span_out) return RCBF_E_BAD_MODE;
    if (!goal_met) traj_mask &= ~RCBF_TRAJ_GOAL_MET;  // a null pointer is not recorded, and never advanced
    if (!status_out) traj_mask &= ~RCBF_TRAJ_STATUS;
    if (!traj_mask) traj_pitch = 0;
    if (traj_mask && (traj_pitch < B || traj_pitch % 4 != 0)) return RCBF_E_BAD_SHAPE;
    if ((traj_mask & RCBF_TRAJ_OBS) && (((uintptr_t)obs_out) & 15)) return RCBF_E_BAD_SHAPE;
    if (term && (((uintptr_t)term_obs) & 15)) return RCBF_E_BAD_SHAPE;
    // RCBF_AQL_PROFILE: a completion signal (timestamps) on every packet; RCBF_AQL_PROFILE_ENDS: on the first
    // and the last only, so the run is timed end to end without a signal between steps (each one adds
    // ~1.5 us to its step: profiles/r06/aql_dispatch_signal_cost)
    const bool ends = (flags & RCBF_AQL_PROFILE_ENDS) != 0;
    const bool profiled = (flags & RCBF_AQL_PROFILE) != 0 || ends;
    if (profiled && !q->profiling) return RCBF_E_BAD_MODE;
    DeviceGuard guard(q->device);
    // the launch rcbf_safe_step would make: solver, mode, hazards, workgroup size
    const int solver = prm->solver;
    const int mode = prm->mode;
    const int k = mode == RCBF_MODE_SIMULATED_CARS ? 1 : prm->num_hazards;
    const int bs = solver == RCBF_SOLVER_ACTIVE_SET ? block_for_envs(B) : 256;
    const KernelInfo* ki = find_kernel(q, safe_step_prefix(solver, mode, k, bs, span_out != nullptr));
    if (!ki || ki->kernarg_bytes != sizeof(SafeStepArgs)) return RCBF_E_BAD_MODE;
    const uint64_t groups = (uint64_t)grid_for_envs(B, bs);

    // The fused form: one dispatch of k_safe_steps per chunk of at most kFusedChunk steps, each lane running
    // its env's steps back to back.  It needs the whole-plan view this call has (every action known before
    // the run) and nothing per step from outside: no stamps, no per-dispatch timestamps, no study fences.
    // The kernel loads step j + 1's action before step j's stores, so a u_RL buffer that overlaps anything
    // the steps write keeps the plan in the per-step form (and its behaviour).
    constexpr int32_t kPerStepFlags =
        RCBF_AQL_PROFILE | RCBF_AQL_STUDY_MID_NOFENCE | RCBF_AQL_STUDY_MID_NOACQ | RCBF_AQL_STUDY_MID_NOREL |
        RCBF_AQL_PER_STEP;
    const bool cars = mode == RCBF_MODE_SIMULATED_CARS;
    const size_t ns = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NS : Dims<RCBF_MODE_UNICYCLE, 1>::NS;
    const size_t no = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NO : Dims<RCBF_MODE_UNICYCLE, 1>::NO;
    const size_t nu = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NU : Dims<RCBF_MODE_UNICYCLE, 1>::NU;
    // bytes of one row of each output's (K, P, w) array; 0: not recorded (written in place)
    const int64_t P = traj_pitch;
    const int64_t row_obs = traj_mask & RCBF_TRAJ_OBS ? P * (int64_t)no * 4 : 0;
    const int64_t row_u = traj_mask & RCBF_TRAJ_U ? P * (int64_t)nu * 4 : 0;
    const int64_t row_rew = traj_mask & RCBF_TRAJ_REWARD ? P * 4 : 0;
    const int64_t row_cost = traj_mask & RCBF_TRAJ_COST ? P * 4 : 0;
    const int64_t row_done = traj_mask & RCBF_TRAJ_DONE ? P : 0;
    const int64_t row_goal = traj_mask & RCBF_TRAJ_GOAL_MET ? P : 0;
    const int64_t row_stat = traj_mask & RCBF_TRAJ_STATUS ? P * 4 : 0;
    const int64_t row_term = term ? P * (int64_t)no * 4 : 0;
    const StepIo io{prm,     B,          x,         aux,        step,     episode,    mu,
                    sigma,   prior_cols, obs_out,   u_out,      reward,   cost,       done,
                    goal_met, status_out, fail_flag, auto_reset, seed,     env_offset, row_obs,
                    row_u,   row_rew,    row_cost,  row_done,   row_goal, row_stat};
    const KernelInfo* kf = nullptr;
    // a plan that keeps the terminal observation is fused at any K (k_safe_steps_term with steps = 1 included)
    if (q->fused && (K > 1 || term) && solver == RCBF_SOLVER_ACTIVE_SET && !span_out && !(flags & kPerStepFlags))
        kf = term        ? (q->term ? find_kernel(q, safe_steps_term_prefix(mode, k, bs)) : nullptr)
             : traj_mask ? (q->traj ? find_kernel(q, safe_steps_traj_prefix(mode, k, bs)) : nullptr)
                         : find_kernel(q, safe_steps_prefix(mode, k, bs));
    if (kf && kf->kernarg_bytes != (term        ? sizeof(SafeStepsTermArgs)
                                    : traj_mask ? sizeof(SafeStepsTrajArgs)
                                                : sizeof(SafeStepsArgs)))
        kf = nullptr;
    if (kf) {
        const size_t n = (size_t)B;
        // a recorded output: the whole (K, P, w) array
        auto ext = [K](int64_t row, size_t in_place) { return row ? (size_t)K * (size_t)row : in_place; };
        const struct {
            const void* p;
            size_t bytes;
        } written[] = {{x, ns * n * 8},
                       {aux, n * 8},
                       {step, n * 4},
                       {episode, n * 4},
                       {obs_out, ext(row_obs, no * n * 4)},
                       {u_out, ext(row_u, nu * n * 4)},
                       {reward, ext(row_rew, n * 4)},
                       {cost, ext(row_cost, n * 4)},
                       {done, ext(row_done, n)},
                       {goal_met, ext(row_goal, n)},
                       {status_out, ext(row_stat, n * 4)},
                       {term_obs, ext(row_term, 0)},
                       {fail_flag, 4}};
        for (int32_t j = 0; j < n_u_rl && kf; ++j)
            for (const auto& w : written)
                if (overlaps(u_rl_seq[j], nu * n * 4, w.p, w.bytes)) {
                    kf = nullptr;
                    break;
                }
    }
    // The cars fused plan's straight-line loop (k_safe_steps_fast, rcbf_safe_steps_fast.hpp) in k_safe_steps's
    // place, same argument block and same results: a plain fused cars plan whose waves are all full and stage
    // their rows through LDS (B % 64 == 0, a 16-byte aligned observation buffer), with the optional buffers as
    // BatchedEnv passes them for cars (no goal_met, no status_out; episode and fail_flag).  Anything else, a code
    // object without those kernels, and RCBF_AQL_FUSED_LOOP take k_safe_steps as before.
    bool fast = false;
    if (kf && q->fast && cars && !term && !traj_mask && K > 1 && B % 64 == 0 && !(((uintptr_t)obs_out) & 15) &&
        !goal_met && !status_out && episode && fail_flag && !(flags & RCBF_AQL_FUSED_LOOP)) {
        const KernelInfo* kfast = find_kernel(q, safe_steps_fast_prefix(bs));
        if (kfast && kfast->kernarg_bytes == sizeof(SafeStepsArgs)) {
            kf = kfast;
            fast = true;
        }
    }
    if (term && !kf) return RCBF_E_BAD_MODE;  // no per-step form keeps the terminal observation
    const int32_t npkt = kf ? (K + kFusedChunk - 1) / kFusedChunk : K;

    auto* p = new rcbf_aql_plan();
    p->q = q;
    p->device = q->device;
    p->K = K;
    p->profiled = ends ? 2 : profiled ? 1 : 0;
    p->form = fast ? RCBF_AQL_FORM_FUSED_FAST : kf ? RCBF_AQL_FORM_FUSED : RCBF_AQL_FORM_PER_STEP;
    // the fused form's table of the n_u_rl action pointers follows the argument blocks
    const size_t table_off = (size_t)npkt * kArgStride;
    std::vector<unsigned char> host(table_off + (kf ? (size_t)n_u_rl * sizeof(const float*) : 0), 0);
    int rc = (int)hipMalloc(&p->kernargs, host.size());
    if (kf) std::memcpy(host.data() + table_off, u_rl_seq, (size_t)n_u_rl * sizeof(const float*));
    for (int32_t j = 0; j < npkt && !rc; ++j) {
        // the row the packet's first step writes of every recorded output: chunk j starts at step j kFusedChunk
        const int64_t r0 = kf ? (int64_t)j * kFusedChunk : (int64_t)j;
        if (kf) {
            SafeStepsTermArgs ea;
            std::memset(&ea, 0, sizeof ea);
            SafeStepsTrajArgs& ta = ea.t;
            SafeStepsArgs& a = ta.s;
            ea.term_obs = rows_on(term_obs, r0, row_term);
            ta.traj_mask = traj_mask;
            ta.traj_pitch = traj_pitch;
            io.fill(a, r0);
            a.u_tab = reinterpret_cast<const float* const*>(static_cast<unsigned char*>(p->kernargs) + table_off);
            a.n_u = n_u_rl;
            // chunk j: steps j kFusedChunk ... of the plan; its first step reads u_rl_seq[that index % n_u_rl]
            a.steps = std::min<int32_t>(kFusedChunk, K - j * kFusedChunk);
            a.ju0 = (int32_t)(((int64_t)j * kFusedChunk) % n_u_rl);
            // k_safe_steps reads the first sizeof(SafeStepsArgs) bytes, k_safe_steps_traj the first
            // sizeof(SafeStepsTrajArgs), k_safe_steps_term all of it
            std::memcpy(host.data() + (size_t)j * kArgStride, &ea, sizeof ea);
            continue;
        }
        SafeStepArgs a;
        io.fill(a, r0);
        a.u_rl = u_rl_seq[j % n_u_rl];
        // step j's stamps: its own block of 4 ceil(B / 64) words
        a.stamp_buf = span_out ? reinterpret_cast<unsigned long long*>(span_out) + (size_t)j * 4 * ((B + 63) / 64)
                               : nullptr;
        std::memcpy(host.data() + (size_t)j * kArgStride, &a, sizeof a);
    }
    if (!rc) rc = (int)hipMemcpy(p->kernargs, host.data(), host.size(), hipMemcpyHostToDevice);
    // ends: a signal on the first and on the last packet; when they are the same packet, one signal is both
    // (with two, the last one is on no packet and rcbf_aql_run would wait for it until its timeout)
    const int nsig = p->profiled == 1 ? npkt : p->profiled == 2 ? (npkt > 1 ? 2 : 1) : 1;
    for (int j = 0; !rc && j < nsig; ++j) {
        hsa_signal_t s;
        rc = hsa_rc(hsa_signal_create(1, 0, nullptr, &s));
        if (!rc) p->sig.push_back(s);
    }
    if (rc) {
        rcbf_aql_plan_free(p);
        return rc;
    }
    const KernelInfo* kd = kf ? kf : ki;
    p->pkt.resize(npkt);
    for (int32_t j = 0; j < npkt; ++j) {
        hsa_kernel_dispatch_packet_t& d = p->pkt[j];
        std::memset(&d, 0, sizeof d);
        int acq = j == 0 && (flags & RCBF_AQL_FIRST_ACQUIRE_SYSTEM) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
        int rel =
            j == npkt - 1 && !(flags & RCBF_AQL_LAST_RELEASE_AGENT) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
        if ((flags & (RCBF_AQL_STUDY_MID_NOFENCE | RCBF_AQL_STUDY_MID_NOACQ)) && j > 0) acq = HSA_FENCE_SCOPE_NONE;
        if ((flags & (RCBF_AQL_STUDY_MID_NOFENCE | RCBF_AQL_STUDY_MID_NOREL)) && j < npkt - 1)
            rel = HSA_FENCE_SCOPE_NONE;
        d.header = (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) |
                              (1 << HSA_PACKET_HEADER_BARRIER) | (acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                              (rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
        d.setup = (uint16_t)(1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS);
        d.workgroup_size_x = (uint16_t)bs;
        d.workgroup_size_y = 1;
        d.workgroup_size_z = 1;
        d.grid_size_x = (uint32_t)(groups * (uint64_t)bs);
        d.grid_size_y = 1;
        d.grid_size_z = 1;
        d.private_segment_size = kd->private_bytes;
        d.group_segment_size = kd->group_bytes;
        d.kernel_object = kd->object;
        d.kernarg_address = static_cast<unsigned char*>(p->kernargs) + (size_t)j * kArgStride;
        if (p->profiled == 1)
            d.completion_signal = p->sig[j];
        else if (p->profiled == 2 && (j == 0 || j == npkt - 1))
            d.completion_signal = j == 0 ? p->sig.front() : p->sig.back();
        else if (j == npkt - 1)
            d.completion_signal = p->sig[0];
        else
            d.completion_signal.handle = 0;
    }
    *out = p;
    return 0;
}

int rcbf_aql_safe_step_plan(rcbf_aql* q, const rcbf_params* prm, int64_t B, int32_t K, double* x, double* aux,
                            int32_t* step, uint32_t* episode, const float* const* u_rl_seq, int32_t n_u_rl,
                            const float* mu, const float* sigma, int32_t prior_cols, float* obs_out, float* u_out,
                            float* reward, float* cost, uint8_t* done, uint8_t* goal_met, int32_t* status_out,
                            int32_t* fail_flag, int32_t auto_reset, uint64_t seed, int64_t env_offset,
                            uint64_t* span_out, int32_t flags, rcbf_aql_plan** out) {
    return build_safe_step_plan(q, prm, B, K, x, aux, step, episode, u_rl_seq, n_u_rl, mu, sigma, prior_cols, obs_out,
                                u_out, reward, cost, done, goal_met, status_out, fail_flag, auto_reset, seed,
                                env_offset, span_out, flags, 0, 0, nullptr, out);
}

int rcbf_aql_safe_step_traj_plan(rcbf_aql* q, const rcbf_params* prm, int64_t B, int32_t K, double* x, double* aux,
                                 int32_t* step, uint32_t* episode, const float* const* u_rl_seq, int32_t n_u_rl,
                                 const float* mu, const float* sigma, int32_t prior_cols, float* obs_out,
                                 float* u_out, float* reward, float* cost, uint8_t* done, uint8_t* goal_met,
                                 int32_t* status_out, int32_t* fail_flag, int32_t auto_reset, uint64_t seed,
                                 int64_t env_offset, uint64_t* span_out, int32_t flags, int32_t traj_mask,
                                 int64_t traj_pitch, rcbf_aql_plan** out) {
    return build_safe_step_plan(q, prm, B, K, x, aux, step, episode, u_rl_seq, n_u_rl, mu, sigma, prior_cols, obs_out,
                                u_out, reward, cost, done, goal_met, status_out, fail_flag, auto_reset, seed,
                                env_offset, span_out, flags, traj_mask, traj_pitch, nullptr, out);
}

int rcbf_aql_safe_step_term_plan(rcbf_aql* q, const rcbf_params* prm, int64_t B, int32_t K, double* x, double* aux,
                                 int32_t* step, uint32_t* episode, const float* const* u_rl_seq, int32_t n_u_rl,
                                 const float* mu, const float* sigma, int32_t prior_cols, float* obs_out,
                                 float* u_out, float* reward, float* cost, uint8_t* done, uint8_t* goal_met,
                                 int32_t* status_out, int32_t* fail_flag, int32_t auto_reset, uint64_t seed,
                                 int64_t env_offset, uint64_t* span_out, int32_t flags, int32_t traj_mask,
                                 int64_t traj_pitch, float* term_obs, rcbf_aql_plan** out) {
    return build_safe_step_plan(q, prm, B, K, x, aux, step, episode, u_rl_seq, n_u_rl, mu, sigma, prior_cols, obs_out,
                                u_out, reward, cost, done, goal_met, status_out, fail_flag, auto_reset, seed,
                                env_offset, span_out, flags, traj_mask, traj_pitch, term_obs, out);
}

int rcbf_aql_closed_loop_plan(rcbf_aql* q, const rcbf_params* prm, int64_t B, int32_t K, double* x, double* aux,
                              int32_t* step, uint32_t* episode, float* u_rl_buf, const float* mu, const float* sigma,
                              int32_t prior_cols, float* obs_out, float* u_out, float* reward, float* cost,
                              uint8_t* done, uint8_t* goal_met, int32_t* status_out, int32_t* fail_flag,
                              int32_t auto_reset, uint64_t seed, int64_t env_offset, uint64_t* span_out,
                              int32_t flags, int32_t traj_mask, int64_t traj_pitch, float* term_obs,
                              const float* obs_in, const float* packed, int32_t n_o, int32_t n_u, int32_t hidden,
                              int32_t mode, uint64_t policy_seed, const uint64_t* counter_word,
                              int64_t policy_env_offset, rcbf_aql_plan** out) {
    if (!q || !out) return RCBF_E_NULL;
    *out = nullptr;
    if (int e = check_prm(prm)) return e;
    // 2 K packets, counted in an int32
    if (B <= 0 || K <= 0 || B > INT32_MAX || K > INT32_MAX / 2) return RCBF_E_BAD_SHAPE;
    if (!x || !aux || !step || !obs_out || !u_out || !reward || !cost || !done) return RCBF_E_NULL;
    if (!u_rl_buf || !obs_in || !packed) return RCBF_E_NULL;
    if ((((uintptr_t)obs_out) & 7) || (((uintptr_t)x) & 15)) return RCBF_E_BAD_SHAPE;
    if (prior_cols && prm->mode == RCBF_MODE_SIMULATED_CARS && mu) return RCBF_E_BAD_SHAPE;
    // per-dispatch timestamps, stamps and the study fences belong to the plans of steps alone
    constexpr int32_t kRefused =
        RCBF_AQL_PROFILE | RCBF_AQL_STUDY_MID_NOFENCE | RCBF_AQL_STUDY_MID_NOACQ | RCBF_AQL_STUDY_MID_NOREL;
    if (span_out || (flags & kRefused)) return RCBF_E_BAD_MODE;
    // the trajectory contract, as build_safe_step_plan checks it
    const bool term = (traj_mask & RCBF_TRAJ_TERM_OBS) != 0;
    if (term != (term_obs != nullptr)) return RCBF_E_BAD_MODE;
    if (traj_mask & ~(kTrajAll | RCBF_TRAJ_TERM_OBS)) return RCBF_E_BAD_MODE;
    if (!goal_met) traj_mask &= ~RCBF_TRAJ_GOAL_MET;
    if (!status_out) traj_mask &= ~RCBF_TRAJ_STATUS;
    if (!traj_mask) traj_pitch = 0;
    if (traj_mask && (traj_pitch < B || traj_pitch % 4 != 0)) return RCBF_E_BAD_SHAPE;
    if ((traj_mask & RCBF_TRAJ_OBS) && (((uintptr_t)obs_out) & 15)) return RCBF_E_BAD_SHAPE;
    if (term && (((uintptr_t)term_obs) & 15)) return RCBF_E_BAD_SHAPE;
    // the policy's contract, as rcbf_policy_act checks it
    if (!policy_shape_ok(n_o, n_u, hidden) || policy_env_offset < 0) return RCBF_E_BAD_SHAPE;
    if (mode != RCBF_POLICY_MEAN && mode != RCBF_POLICY_SAMPLE) return RCBF_E_BAD_MODE;
    if ((((uintptr_t)packed) & 15) || (((uintptr_t)obs_in) & 3) || (((uintptr_t)u_rl_buf) & 3) ||
        (((uintptr_t)counter_word) & 7))
        return RCBF_E_BAD_SHAPE;
    const bool cars = prm->mode == RCBF_MODE_SIMULATED_CARS;
    const size_t ns = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NS : Dims<RCBF_MODE_UNICYCLE, 1>::NS;
    const size_t no = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NO : Dims<RCBF_MODE_UNICYCLE, 1>::NO;
    const size_t nu = cars ? Dims<RCBF_MODE_SIMULATED_CARS, 1>::NU : Dims<RCBF_MODE_UNICYCLE, 1>::NU;
    // the policy reads the env's observation rows and writes the env's action rows
    if ((size_t)n_o != no || (size_t)n_u != nu) return RCBF_E_BAD_SHAPE;
    const bool ends = (flags & RCBF_AQL_PROFILE_ENDS) != 0;
    if (ends && !q->profiling) return RCBF_E_BAD_MODE;
    if (!q->policy) return RCBF_E_BAD_MODE;
    // bytes of one row of each output's (K, P, w) array; 0: not recorded (written in place)
    const int64_t P = traj_pitch;
    const int64_t row_obs = traj_mask & RCBF_TRAJ_OBS ? P * (int64_t)no * 4 : 0;
    const int64_t row_u = traj_mask & RCBF_TRAJ_U ? P * (int64_t)nu * 4 : 0;
    const int64_t row_rew = traj_mask & RCBF_TRAJ_REWARD ? P * 4 : 0;
    const int64_t row_cost = traj_mask & RCBF_TRAJ_COST ? P * 4 : 0;
    const int64_t row_done = traj_mask & RCBF_TRAJ_DONE ? P : 0;
    const int64_t row_goal = traj_mask & RCBF_TRAJ_GOAL_MET ? P : 0;
    const int64_t row_stat = traj_mask & RCBF_TRAJ_STATUS ? P * 4 : 0;
    const int64_t row_term = term ? P * (int64_t)no * 4 : 0;
    const StepIo io{prm,     B,          x,         aux,        step,     episode,    mu,
                    sigma,   prior_cols, obs_out,   u_out,      reward,   cost,       done,
                    goal_met, status_out, fail_flag, auto_reset, seed,     env_offset, row_obs,
                    row_u,   row_rew,    row_cost,  row_done,   row_goal, row_stat};
    {
        // the action buffer is written by every policy packet and read by every step packet: it overlaps nothing
        // else that either of them reads or writes
        const size_t n = (size_t)B;
        auto ext = [K](int64_t row, size_t in_place) { return row ? (size_t)K * (size_t)row : in_place; };
        const int64_t H = hidden, K1 = n_o + (n_o & 1);
        const size_t packed_bytes = (size_t)(H * (K1 + H + 2 + 2 * n_u) + 16) * 4;  // rcbf_policy_packed_floats
        const size_t prior_bytes = (prior_cols ? 3 : ns) * n * 4;
        const struct {
            const void* p;
            size_t bytes;
        } others[] = {{x, ns * n * 8},
                      {aux, n * 8},
                      {step, n * 4},
                      {episode, n * 4},
                      {obs_out, ext(row_obs, no * n * 4)},
                      {u_out, ext(row_u, nu * n * 4)},
                      {reward, ext(row_rew, n * 4)},
                      {cost, ext(row_cost, n * 4)},
                      {done, ext(row_done, n)},
                      {goal_met, ext(row_goal, n)},
                      {status_out, ext(row_stat, n * 4)},
                      {term_obs, ext(row_term, 0)},
                      {fail_flag, 4},
                      {mu, prior_bytes},
                      {sigma, prior_bytes},
                      {obs_in, no * n * 4},
                      {packed, packed_bytes},
                      {counter_word, 8}};
        for (const auto& w : others)
            if (overlaps(u_rl_buf, nu * n * 4, w.p, w.bytes)) return RCBF_E_BAD_SHAPE;
    }
    DeviceGuard guard(q->device);
    const int solver = prm->solver;
    const int k = cars ? 1 : prm->num_hazards;
    const int bs = solver == RCBF_SOLVER_ACTIVE_SET ? block_for_envs(B) : 256;
    // the step packet: k_safe_step with step j's row pointers, or, to keep the terminal observation, a one-step
    // dispatch of k_safe_steps_term (exact active set only) at row offset j
    const KernelInfo* ks = nullptr;
    if (term) {
        if (solver != RCBF_SOLVER_ACTIVE_SET || !q->term) return RCBF_E_BAD_MODE;
        ks = find_kernel(q, safe_steps_term_prefix(prm->mode, k, bs));
        if (!ks || ks->kernarg_bytes != sizeof(SafeStepsTermArgs)) return RCBF_E_BAD_MODE;
    } else {
        ks = find_kernel(q, safe_step_prefix(solver, prm->mode, k, bs, false));
        if (!ks || ks->kernarg_bytes != sizeof(SafeStepArgs)) return RCBF_E_BAD_MODE;
    }
    // the policy packet: the tile rule of rcbf_policy_act; the packet itself carries the dynamic LDS size (nothing
    // like hipFuncSetAttribute applies to a raw dispatch): above 64 KiB from H = 256, inside gfx950's 160 KiB
    const int nrb = B <= 32 * num_cus() ? 1 : 2;
    const KernelInfo* kp = find_kernel(q, policy_step_prefix(mode == RCBF_POLICY_SAMPLE, nrb));
    if (!kp || kp->kernarg_bytes != sizeof(PolicyStepArgs)) return RCBF_E_BAD_MODE;
    const size_t policy_lds = (size_t)kp->group_bytes + policy_lds_bytes(hidden, nrb);
    if (policy_lds > 160 * 1024) return RCBF_E_BAD_SHAPE;
    const uint64_t step_groups = (uint64_t)grid_for_envs(B, bs);
    const uint64_t policy_groups = (uint64_t)((B + 32 * nrb - 1) / (32 * nrb));
    if (policy_groups * 256u > UINT32_MAX) return RCBF_E_BAD_SHAPE;  // a packet's grid is counted in work-items
    const int32_t npkt = 2 * K;

    auto* p = new rcbf_aql_plan();
    p->q = q;
    p->device = q->device;
    p->K = K;
    p->profiled = ends ? 2 : 0;
    // the one-entry action table of the k_safe_steps_term packets follows the argument blocks
    const size_t table_off = (size_t)npkt * kArgStride;
    std::vector<unsigned char> host(table_off + sizeof(const float*), 0);
    int rc = (int)hipMalloc(&p->kernargs, host.size());
    {
        const float* const tab = u_rl_buf;
        std::memcpy(host.data() + table_off, &tab, sizeof tab);
    }
    for (int32_t j = 0; j < K && !rc; ++j) {
        PolicyStepArgs pa;
        std::memset(&pa, 0, sizeof pa);
        pa.packed = packed;
        pa.n_o = n_o;
        pa.n_u = n_u;
        pa.H = hidden;
        pa.B = B;
        // the observation step j - 1 left: its row of a recorded obs array, else the buffer every step overwrites
        pa.obs = j == 0 ? obs_in : row_obs ? rows_on(obs_out, (int64_t)j - 1, row_obs) : obs_out;
        pa.u_rl = u_rl_buf;
        pa.seed = policy_seed;
        pa.counter_word = counter_word;
        pa.counter_add = (uint64_t)j;
        pa.env_offset = policy_env_offset;
        std::memcpy(host.data() + (size_t)(2 * j) * kArgStride, &pa, sizeof pa);
        unsigned char* const dst = host.data() + (size_t)(2 * j + 1) * kArgStride;
        if (term) {
            SafeStepsTermArgs ea;
            std::memset(&ea, 0, sizeof ea);
            SafeStepsTrajArgs& ta = ea.t;
            SafeStepsArgs& a = ta.s;
            ea.term_obs = rows_on(term_obs, j, row_term);
            ta.traj_mask = traj_mask;
            ta.traj_pitch = traj_pitch;
            io.fill(a, j);
            // one step, its action the table's only entry
            a.u_tab = reinterpret_cast<const float* const*>(static_cast<unsigned char*>(p->kernargs) + table_off);
            a.n_u = 1;
            a.steps = 1;
            a.ju0 = 0;
            std::memcpy(dst, &ea, sizeof ea);
        } else {
            SafeStepArgs a;
            io.fill(a, j);
            a.u_rl = u_rl_buf;
            std::memcpy(dst, &a, sizeof a);
        }
    }
    if (!rc) rc = (int)hipMemcpy(p->kernargs, host.data(), host.size(), hipMemcpyHostToDevice);
    // ends: a signal on the first packet and one on the last; else one, on the last
    for (int j = 0; !rc && j < (ends ? 2 : 1); ++j) {
        hsa_signal_t s;
        rc = hsa_rc(hsa_signal_create(1, 0, nullptr, &s));
        if (!rc) p->sig.push_back(s);
    }
    if (rc) {
        rcbf_aql_plan_free(p);
        return rc;
    }
    p->pkt.resize(npkt);
    for (int32_t j = 0; j < npkt; ++j) {
        const bool is_policy = (j & 1) == 0;
        const KernelInfo* kd = is_policy ? kp : ks;
        hsa_kernel_dispatch_packet_t& d = p->pkt[j];
        std::memset(&d, 0, sizeof d);
        // the fences of the per-step form: agent scope between packets (the action and the observation pass
        // through memory from one packet to the next), system-scope release on the last
        const int acq =
            j == 0 && (flags & RCBF_AQL_FIRST_ACQUIRE_SYSTEM) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
        const int rel =
            j == npkt - 1 && !(flags & RCBF_AQL_LAST_RELEASE_AGENT) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
        d.header = (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) |
                              (1 << HSA_PACKET_HEADER_BARRIER) | (acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                              (rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
        d.setup = (uint16_t)(1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS);
        d.workgroup_size_x = (uint16_t)(is_policy ? 256 : bs);
        d.workgroup_size_y = 1;
        d.workgroup_size_z = 1;
        d.grid_size_x = (uint32_t)(is_policy ? policy_groups * 256u : step_groups * (uint64_t)bs);
        d.grid_size_y = 1;
        d.grid_size_z = 1;
        d.private_segment_size = kd->private_bytes;
        d.group_segment_size = is_policy ? (uint32_t)policy_lds : kd->group_bytes;
        d.kernel_object = kd->object;
        d.kernarg_address = static_cast<unsigned char*>(p->kernargs) + (size_t)j * kArgStride;
        if (j == npkt - 1)
            d.completion_signal = p->sig.back();
        else if (ends && j == 0)
            d.completion_signal = p->sig.front();
        else
            d.completion_signal.handle = 0;
    }
    *out = p;
    return 0;
}

}  // extern "C"

namespace {

// Copy packets j, j + 1, ... of plan p into its queue's ring, as many as the ring has room for right now,
// and ring the doorbell once for them; returns the new j (unchanged when the ring is full).
int32_t feed(rcbf_aql_plan* p, int32_t j) {
    hsa_queue_t* queue = p->q->queue;
    const uint64_t mask = queue->size - 1;
    auto* ring = static_cast<hsa_kernel_dispatch_packet_t*>(queue->base_address);
    const uint64_t rd = hsa_queue_load_read_index_scacquire(queue);
    const uint64_t wr = hsa_queue_load_write_index_relaxed(queue);
    const uint64_t room = queue->size - (wr - rd);
    if (room == 0) return j;
    const int32_t n = (int32_t)std::min<uint64_t>(room, (uint64_t)((int32_t)p->pkt.size() - j));
    const uint64_t w = hsa_queue_add_write_index_relaxed(queue, (uint64_t)n);
    for (int32_t i = 0; i < n; ++i) {
        hsa_kernel_dispatch_packet_t* slot = &ring[(w + i) & mask];
        const hsa_kernel_dispatch_packet_t& src = p->pkt[j + i];
        std::memcpy(reinterpret_cast<char*>(slot) + 4, reinterpret_cast<const char*>(&src) + 4, sizeof(src) - 4);
        __atomic_store_n(reinterpret_cast<uint32_t*>(slot), (uint32_t)src.header | ((uint32_t)src.setup << 16),
                         __ATOMIC_RELEASE);
    }
    hsa_signal_store_screlease(queue->doorbell_signal, (hsa_signal_value_t)(w + n - 1));
    return j + n;
}

// Busy-wait for plan p's last completion signal (a synchronous step: the host has nothing else to do, and
// a sleeping wait adds its wake-up latency to every call).
int wait_done(rcbf_aql_plan* p, uint64_t t_end) {
    const hsa_signal_t last = p->sig.back();
    for (;;) {
        const hsa_signal_value_t v =
            hsa_signal_wait_scacquire(last, HSA_SIGNAL_CONDITION_LT, 1, 1000000, HSA_WAIT_STATE_ACTIVE);
        if (v < 1) return p->q->queue_error.load() ? RCBF_E_HSA : 0;
        if (p->q->queue_error.load()) return RCBF_E_HSA;
        if (now_ns() > t_end) return RCBF_E_TIMEOUT;
    }
}

}  // namespace

extern "C" {

int rcbf_aql_run(rcbf_aql_plan* p, uint64_t timeout_us) {
    if (!p || !p->q || !p->q->queue) return RCBF_E_NULL;
    if (p->q->queue_error.load()) return RCBF_E_HSA;
    for (auto& s : p->sig) hsa_signal_store_relaxed(s, 1);
    const uint64_t t_end = now_ns() + (timeout_us ? timeout_us : 10000000ull) * 1000ull;
    // as many packets as the ring has room for (all of them unless there are more than the ring holds),
    // then the rest as the packet processor frees slots
    for (int32_t j = 0, n = (int32_t)p->pkt.size(); j < n;) {
        const int32_t nj = feed(p, j);
        if (nj == j) {
            if (p->q->queue_error.load()) return RCBF_E_HSA;
            if (now_ns() > t_end) return RCBF_E_TIMEOUT;
            _mm_pause();
        }
        j = nj;
    }
    return wait_done(p, t_end);
}

int rcbf_aql_plan_times(const rcbf_aql_plan* p, uint64_t* start_end_ns) {
    if (!p || !start_end_ns) return RCBF_E_NULL;
    if (!p->profiled) return RCBF_E_BAD_MODE;
    uint64_t freq = 0;
    hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &freq);
    if (!freq) return RCBF_E_HSA;
    for (int32_t j = 0; j < p->K; ++j) {
        hsa_amd_profiling_dispatch_time_t t;
        hsa_signal_t sg;
        if (p->profiled == 2) {
            // only the first and the last packet carry a signal: the first packet's times in row 0, the
            // last packet's in row K - 1 (one packet, fused or K = 1: both rows are that packet's)
            start_end_ns[2 * j] = start_end_ns[2 * j + 1] = 0;
            if (j != 0 && j != p->K - 1) continue;
            sg = j == 0 ? p->sig.front() : p->sig.back();
        } else {
            sg = p->sig[j];  // a per-dispatch profile is always the per-step form: packet j is step j
        }
        if (hsa_amd_profiling_get_dispatch_time(p->q->agent, sg, &t) != HSA_STATUS_SUCCESS) return RCBF_E_HSA;
        if (p->profiled == 2 && p->K == 1 && p->sig.size() > 1) {
            // a one-step closed-loop plan: the row is its two packets', the policy's start to the step's end
            hsa_amd_profiling_dispatch_time_t t2;
            if (hsa_amd_profiling_get_dispatch_time(p->q->agent, p->sig.back(), &t2) != HSA_STATUS_SUCCESS)
                return RCBF_E_HSA;
            t.end = t2.end;
        }
        start_end_ns[2 * j] = (uint64_t)((long double)t.start * 1e9L / (long double)freq);
        start_end_ns[2 * j + 1] = (uint64_t)((long double)t.end * 1e9L / (long double)freq);
    }
    return 0;
}

int rcbf_aql_plan_dispatches(const rcbf_aql_plan* p) { return p ? (int)p->pkt.size() : RCBF_E_NULL; }

int rcbf_aql_plan_form(const rcbf_aql_plan* p) { return p ? p->form : RCBF_E_NULL; }

int rcbf_aql_plan_free(rcbf_aql_plan* p) {
    if (!p) return 0;
    if (p->kernargs) {
        DeviceGuard guard(p->device);
        (void)hipFree(p->kernargs);
    }
    for (auto& s : p->sig) hsa_signal_destroy(s);
    delete p;
    return 0;
}

}  // extern "C"
