"""The fused safe step on the library's own AQL queue (csrc/rcbf_aql.hip).

`AqlQueue(device)` owns one user-mode HSA queue on a HIP device and the
code object the HIP path launches the fused step from (librcbf_steps.co,
identical machine code).  `AqlQueue.safe_step_plan(env, u_rl_seq, layer, ...)`
is the AQL analogue of capturing K `BatchedEnv.safe_step` calls into a
hipGraph: the K kernel-argument blocks go to device memory once, the K
dispatch packets are pre-built, and `plan.run()` submits them with one
doorbell and returns when the K steps have completed -- a synchronous
env.step() (main.py:93-95, sac_cbf.py:218-238) of K steps.

A plan of K > 1 steps with the exact solver is built in the FUSED form: one
dispatch in which each lane runs its env's K steps back to back (every step
still stores everything a step stores), without the fence and the state
re-load between two dispatches.  `plan.dispatches` tells which form a plan
took (K: per step; 1 per 4096 steps: fused); `fused=False`, a span buffer,
`profile=True` or a u_RL buffer that overlaps an output keep the per-step form.
A fused plain plan of the cars env whose waves are all full (B % 64 == 0, the
observation buffer 16-byte aligned) runs the straight-line loop
(k_safe_steps_fast, csrc/rcbf_safe_steps_fast.hpp), bit for bit the same steps;
`fast=False` keeps k_safe_steps, and `plan.form` names the kernel a plan took
("per_step", "fused", "fused_fast").

A TRAJECTORY plan (`trajectory=True`, or a dict from
`BatchedEnv.make_trajectory`) keeps every step's outputs: step j writes row j
of each recorded field's (K, B[, w]) array instead of overwriting the one
(B[, w]) buffer -- what the warm-up phase (main.py:88-107) and evaluation
rollouts need from steps whose actions are known beforehand.  It takes the
same two forms (fused: the k_safe_steps_traj kernels).  `plan.trajectory` is
the dict; after `run()` the env and the outputs dict are as after a plain plan.
With a "term_obs" field (`env.make_trajectory(K, fields + ("term_obs",))`) the
plan also keeps, at [j][i] of that array, the TERMINAL observation of an env
that step j auto-resets (obs[j][i] is then the next episode's first row);
every other element of the array is left as it was.  Such a plan is always
fused (the k_safe_steps_term kernels, K = 1 included): where it would have to
be per-step, safe_step_plan raises.  `ReplayMemory.push_trajectory` packs the
result into replay records.

A CLOSED-LOOP plan (`AqlQueue.closed_loop_plan(env, policy, layer, K, ...)`)
is for the steps whose actions are NOT known beforehand: a DevicePolicy
computes step j's action from the observation step j - 1 left.  It is 2K
packets, the policy's kernel (rcbf::k_policy_step, librcbf_policy.co) before
every step, with the fences of the per-step form; it records trajectories
("term_obs" included) like the plans above, and everything is bit for bit what
K times policy.act() then env.safe_step() compute through the HIP launch path.

The queue is not a HIP stream: `run()` first waits for all HIP work queued
on the env's device unless `sync_hip=False` is
passed by a caller that has synchronised itself (bench.py's timed region
follows torch.cuda.synchronize()).
"""
import ctypes
import weakref

import torch

from . import _lib

PROFILE = 1  # RCBF_AQL_PROFILE
PROFILE_ENDS = 64  # RCBF_AQL_PROFILE_ENDS: timestamps of the first and last dispatch only
PER_STEP = 128  # RCBF_AQL_PER_STEP: K dispatches even where the fused form applies
FUSED_LOOP = 256  # RCBF_AQL_FUSED_LOOP: a fused cars plan keeps k_safe_steps where k_safe_steps_fast applies
FORMS = ("per_step", "fused", "fused_fast")  # RCBF_AQL_FORM_*: AqlPlan.form
# RCBF_TRAJ_*: the outputs a trajectory plan records
TRAJ_OBS, TRAJ_U, TRAJ_REWARD, TRAJ_COST, TRAJ_DONE, TRAJ_GOAL_MET, TRAJ_STATUS = 1, 2, 4, 8, 16, 32, 64
TRAJ_BITS = {"obs": TRAJ_OBS, "u": TRAJ_U, "reward": TRAJ_REWARD, "cost": TRAJ_COST, "done": TRAJ_DONE,
             "goal_met": TRAJ_GOAL_MET, "status": TRAJ_STATUS}
# RCBF_TRAJ_TERM_OBS: a side output, not one of the step's outputs (so not in TRAJ_BITS): the observation of the
# post-step state of a step that auto-resets, before the reset (trajectory["term_obs"])
TRAJ_TERM_OBS = 128


def _bind():
    return _lib.load()


def _check(rc, what):
    _lib.check(rc, what)


class AqlQueue:
    """One AQL queue on HIP device `device` (int or torch.device)."""

    def __init__(self, device=None, profile=False, code_object=None):
        lib = _bind()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("AqlQueue needs a HIP device")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.profile = bool(profile)
        h = ctypes.c_void_p()
        _check(lib.rcbf_aql_open(self.device.index, code_object.encode() if code_object else None,
                                 PROFILE if profile else 0, ctypes.byref(h)), "rcbf_aql_open")
        self._h = h
        self._plans = weakref.WeakSet()  # live plans: freed before the queue (they point into it)
        self._fin = weakref.finalize(self, lib.rcbf_aql_close, h)

    @property
    def handle(self):
        if not self._fin.alive:
            raise RuntimeError("the AQL queue is closed")
        return self._h

    def kernel_count(self):
        return int(_lib.load().rcbf_aql_kernel_count(self.handle))

    def close(self):
        for p in list(self._plans):
            p.free()
        self._fin()

    def safe_step_plan(self, env, u_rl_seq, layer, steps=None, mean=None, sigma=None, outputs=None,
                       auto_reset=True, prior_layout="rows", span=None, profile=False, fence_flags=0, fused=None,
                       trajectory=None, fast=None):
        """K = steps (default len(u_rl_seq)) fused safe steps of `env` with
        `layer`, step j reading u_rl_seq[j % len(u_rl_seq)]: the same
        arguments and results as env.safe_step_seq (span: the measurement
        instantiation of env.safe_step_span, step j stamping span[j]).
        fused: None or True leave the plan's form to the library (fused where
        it applies, see the module docstring); False asks for K dispatches.
        fast: None or True leave the fused cars plan's kernel to the library;
        False keeps k_safe_steps (RCBF_AQL_FUSED_LOOP).
        trajectory: None (a plain plan), True (record every field of
        env.TRAJECTORY_FIELDS, allocated here) or a dict of (K', B[, w])
        views, K' >= K, of pitch-padded arrays as env.make_trajectory
        returns them, whose keys select the recorded fields: step j writes
        row j of each (on a step that resets, obs[j] is the next episode's
        first observation, and term_obs[j], if that field is there, the
        finished episode's last).  Not with span; with "term_obs" the plan
        must be fused (module docstring)."""
        if env.device != self.device:
            raise ValueError(f"env on {env.device}, queue on {self.device}")
        o = outputs if outputs is not None else env.make_outputs()
        us = [env._u_arg(u) for u in u_rl_seq]
        if not us:
            raise ValueError("u_rl_seq is empty")
        K = len(us) if steps is None else int(steps)
        if prior_layout not in ("rows", "cols"):
            raise ValueError(f"prior_layout must be 'rows' or 'cols', got {prior_layout!r}")
        cols = prior_layout == "cols"
        if cols:
            if mean is not None and env.dynamics_mode == "SimulatedCars":
                raise ValueError("the cars CBF rows read no mean (diff_cbf_qp.py:298-299): pass mean=None")
            mean, sigma = env._prior_cols_arg(mean, "mean"), env._prior_cols_arg(sigma, "sigma")
        else:
            mean, sigma = env._prior_arg(mean, "mean"), env._prior_arg(sigma, "sigma")
        if span is not None:
            nw = (env.num_envs + 63) // 64
            if not (torch.is_tensor(span) and span.dtype == torch.int64 and span.device == env.device
                    and span.is_contiguous() and span.numel() >= 4 * nw * K):
                raise ValueError(f"span must be a contiguous int64 tensor of >= {4 * nw * K} entries "
                                 f"(K blocks of ceil(B / 64) x 4) on {env.device}")
        a = env._step_args(layer, o, auto_reset)
        arr = (ctypes.c_void_p * len(us))(*[u.data_ptr() for u in us])
        h = ctypes.c_void_p()
        flags = ((PROFILE if profile else 0) | (PER_STEP if fused is False else 0) |
                 (FUSED_LOOP if fast is False else 0) | int(fence_flags))
        head = (self.handle, ctypes.byref(layer._prm), env.num_envs, K, *[v or None for v in a[2:6]], arr, len(us),
                None if mean is None else mean.data_ptr(), None if sigma is None else sigma.data_ptr(), int(cols))
        tail = (*a[17:20], None if span is None else span.data_ptr(), flags)
        traj = None
        if trajectory is not None and trajectory is not False:
            if span is not None:
                raise ValueError("a trajectory plan takes no span buffer")
            traj = env.make_trajectory(K) if trajectory is True else dict(trajectory)
            mask, pitch = _trajectory_args(env, traj, K)
            term = traj.get("term_obs")
            if term is not None:
                why = _term_plan_refusal(env, layer, us, term, K, pitch, profile, fused, fence_flags)
                if why:
                    raise ValueError(f"a trajectory plan with term_obs is always fused, but {why}")
            # a[9:17]: obs, u, reward, cost, done, goal_met, status, fail_flag -- a recorded field's pointer is
            # its array's base; the cars goal_met is never recorded (env._step_args passes none either)
            outs = list(a[9:17])
            for j, f in enumerate(("obs", "u", "reward", "cost", "done", "goal_met", "status")):
                if mask & TRAJ_BITS[f]:
                    outs[j] = traj[f].data_ptr()
            with torch.cuda.device(self.device):
                if term is not None:
                    _check(_lib.load().rcbf_aql_safe_step_term_plan(
                        *head, *[v or None for v in outs], *tail, mask | TRAJ_TERM_OBS, pitch, term.data_ptr(),
                        ctypes.byref(h)), "rcbf_aql_safe_step_term_plan")
                else:
                    _check(_lib.load().rcbf_aql_safe_step_traj_plan(
                        *head, *[v or None for v in outs], *tail, mask, pitch, ctypes.byref(h)),
                        "rcbf_aql_safe_step_traj_plan")
        else:
            with torch.cuda.device(self.device):
                _check(_lib.load().rcbf_aql_safe_step_plan(*head, *[v or None for v in a[9:17]], *tail,
                                                           ctypes.byref(h)), "rcbf_aql_safe_step_plan")
        # the plan holds raw pointers: keep every tensor it reads or writes alive with it
        keep = (env, layer, o, us, mean, sigma, span, traj)
        plan = AqlPlan(self, h, K, keep, bool(profile), env, traj)
        self._plans.add(plan)
        return plan

    def closed_loop_plan(self, env, policy, layer, steps, evaluate=False, mean=None, sigma=None, outputs=None,
                         auto_reset=True, prior_layout="rows", trajectory=None, fence_flags=0):
        """K = steps closed-loop steps of `env`: before step j the policy
        (a DevicePolicy) computes the action from the observation step j - 1
        left, as policy.act(env.obs, evaluate, out=u) followed by
        env.safe_step(u, layer, mean, sigma, ...) does, K times, but as 2K
        packets behind one doorbell (rcbf_aql_closed_loop_plan).  Returns a
        ClosedLoopPlan (an AqlPlan): `plan.u_rl` is the (B, n_u) action
        buffer the plan owns (after a run, the last step's policy action);
        `plan.dispatches` is 2K.  trajectory: as in safe_step_plan, "term_obs"
        included (exact solver only).  evaluate=False samples with the
        in-kernel draws of (policy.seed, policy.env_offset + row, counter), the
        counter set per run (ClosedLoopPlan.run).  policy.refresh() between
        runs is seen by the next run: the plan reads the policy's packed
        buffer, whose address does not change.  fence_flags: the fence scopes
        and PROFILE_ENDS (on a queue opened with profile=True)."""
        from .policy import DevicePolicy
        if env.device != self.device:
            raise ValueError(f"env on {env.device}, queue on {self.device}")
        if not isinstance(policy, DevicePolicy):
            raise ValueError("a closed-loop plan needs a DevicePolicy: its packed weights are what the packets read")
        if policy.device != env.device:
            raise ValueError(f"the policy is on {policy.device}, the env on {env.device}")
        if (policy.n_o, policy.n_u) != (env.n_o, env.n_u):
            raise ValueError(f"the policy maps {policy.n_o} observations to {policy.n_u} actions, the env has "
                             f"{env.n_o} and {env.n_u}")
        if not evaluate and not policy.has_log_std:
            raise NotImplementedError("evaluate=False needs a log-std head: the reference's DeterministicPolicy.sample "
                                      "shares one noise vector across rows, which is not reproduced")
        K = int(steps)
        if K <= 0:
            raise ValueError(f"steps must be positive, got {steps}")
        flags = int(fence_flags)
        if flags & (PROFILE | 8 | 16 | 32):
            raise ValueError("a closed-loop plan takes no per-dispatch profile and no study fences "
                             "(PROFILE_ENDS times it end to end)")
        if flags & PROFILE_ENDS and not self.profile:
            raise ValueError("PROFILE_ENDS needs a queue opened with profile=True")
        if prior_layout not in ("rows", "cols"):
            raise ValueError(f"prior_layout must be 'rows' or 'cols', got {prior_layout!r}")
        cols = prior_layout == "cols"
        if cols:
            if mean is not None and env.dynamics_mode == "SimulatedCars":
                raise ValueError("the cars CBF rows read no mean (diff_cbf_qp.py:298-299): pass mean=None")
            mean, sigma = env._prior_cols_arg(mean, "mean"), env._prior_cols_arg(sigma, "sigma")
        else:
            mean, sigma = env._prior_arg(mean, "mean"), env._prior_arg(sigma, "sigma")
        o = outputs if outputs is not None else env.make_outputs()
        a = env._step_args(layer, o, auto_reset)
        outs = list(a[9:17])
        traj, mask, pitch, term = None, 0, 0, None
        if trajectory is not None and trajectory is not False:
            traj = env.make_trajectory(K) if trajectory is True else dict(trajectory)
            mask, pitch = _trajectory_args(env, traj, K)
            term = traj.get("term_obs")
            if term is not None:
                if layer._prm.solver != _lib.SOLVER_ACTIVE_SET:
                    raise ValueError("a plan that records term_obs needs the exact active-set solver, but the "
                                     "layer's solver is another")
                mask |= TRAJ_TERM_OBS
            for j, f in enumerate(("obs", "u", "reward", "cost", "done", "goal_met", "status")):
                if mask & TRAJ_BITS[f]:
                    outs[j] = traj[f].data_ptr()
        u_rl = torch.zeros(env.num_envs, env.n_u, dtype=torch.float32, device=env.device)
        # the draw counter of a sampling plan: one device word, set by run() before the doorbell
        word = None if evaluate else torch.zeros(1, dtype=torch.int64, device=env.device)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(_lib.load().rcbf_aql_closed_loop_plan(
                self.handle, ctypes.byref(layer._prm), env.num_envs, K, *[v or None for v in a[2:6]], u_rl.data_ptr(),
                None if mean is None else mean.data_ptr(), None if sigma is None else sigma.data_ptr(), int(cols),
                *[v or None for v in outs], *a[17:20], None, flags, mask, pitch,
                None if term is None else term.data_ptr(), env.obs.data_ptr(), policy.packed.data_ptr(), policy.n_o,
                policy.n_u, policy.hidden, _lib.POLICY_MEAN if evaluate else _lib.POLICY_SAMPLE,
                policy.seed & 0xFFFFFFFFFFFFFFFF, None if word is None else word.data_ptr(), policy.env_offset,
                ctypes.byref(h)), "rcbf_aql_closed_loop_plan")
        # the plan holds raw pointers: keep every tensor it reads or writes alive with it
        keep = (env, layer, o, u_rl, mean, sigma, None, traj, policy, policy.packed, word)
        plan = ClosedLoopPlan(self, h, K, keep, env, traj, policy, u_rl, word)
        self._plans.add(plan)
        return plan


def _trajectory_args(env, traj, K):
    """(traj_mask, traj_pitch) of a trajectory dict for a K-step plan of
    `env`, after checking every field: a known name, the field's dtype, on
    the env's device, shape (K', B[, w]) with K' >= K, and the strides of a
    [:, :B] view of a dense (K', P[, w]) array, one P for all fields."""
    spec = env._trajectory_spec()
    B = env.num_envs
    mask, pitch = 0, None
    cars = env.dynamics_mode == "SimulatedCars"
    for f, t in traj.items():
        if f not in spec:
            raise ValueError(f"unknown trajectory field {f!r} (one of {sorted(spec)})")
        w, dt = spec[f]
        if not (torch.is_tensor(t) and t.dtype == dt and t.device == env.device):
            raise ValueError(f"trajectory[{f!r}] must be a {dt} tensor on {env.device}")
        want = (B, w) if w else (B,)
        if t.dim() != len(want) + 1 or tuple(t.shape[1:]) != want or t.shape[0] < K:
            raise ValueError(f"trajectory[{f!r}] must have shape (>= {K}, {', '.join(map(str, want))}), "
                             f"got {tuple(t.shape)}")
        ww = w or 1
        st = t.stride()
        if st[1:] != ((w, 1) if w else (1,)) or st[0] % ww or st[0] // ww < B:
            raise ValueError(f"trajectory[{f!r}] must be a [:, :B] view of a dense (K, P{', w' if w else ''}) array "
                             f"(use env.make_trajectory), got strides {st}")
        p = st[0] // ww
        if pitch is not None and p != pitch:
            raise ValueError(f"trajectory[{f!r}] has row pitch {p}, the other fields {pitch}")
        pitch = p
        if f == "goal_met" and cars:
            continue  # never met: stays as make_trajectory zero-filled it
        if f == "term_obs":
            continue  # RCBF_TRAJ_TERM_OBS: set by the caller, which passes the pointer as well
        mask |= TRAJ_BITS[f]
    return mask, (pitch or 0)


def _term_plan_refusal(env, layer, us, term, K, pitch, profile, fused, fence_flags):
    """Why a plan that records term_obs could not take the fused form (the
    library would answer RCBF_E_BAD_MODE), or None."""
    if layer._prm.solver != _lib.SOLVER_ACTIVE_SET:
        return "the layer's solver is not the exact active set"
    if profile:
        return "profile=True asks for per-dispatch timestamps"
    if fused is False:
        return "fused=False asks for the per-step form"
    if int(fence_flags) & (8 | 16 | 32 | PER_STEP | PROFILE):
        return "fence_flags asks for the per-step form"
    lo, n = term.data_ptr(), K * pitch * env.n_o * 4
    for u in us:
        if u.data_ptr() < lo + n and lo < u.data_ptr() + u.numel() * 4:
            return "an action buffer lies inside term_obs's extent"
    return None


class AqlPlan:
    """K pre-built steps of the fused step (see AqlQueue.safe_step_plan)."""

    def __init__(self, queue, handle, K, keep, profiled, env, trajectory=None):
        self.queue, self.K, self.profiled = queue, K, profiled
        self._h, self._keep, self._env = handle, keep, env
        self.trajectory = trajectory  # the dict of a trajectory plan (field -> (K', B[, w]) view), else None
        self._fin = weakref.finalize(self, _lib.load().rcbf_aql_plan_free, handle)

    def run(self, sync_hip=True, timeout_us=0, copy_back=True):
        """Submit the K steps and return when they have completed.  A
        trajectory plan then copies row K - 1 of each recorded field into
        env.obs / the outputs dict, which are then exactly as after a plain
        plan (copy_back=False skips that, for timing)."""
        if sync_hip:
            torch.cuda.synchronize(self.queue.device)
        if not self._fin.alive or not self.queue._fin.alive:
            raise RuntimeError("the AQL plan (or its queue) was freed")
        # ctypes, not the CPython binding: a 20-step run measured the same through both (85.1 / 85.5 us, r06w)
        _check(_lib.load().rcbf_aql_run(self._h, timeout_us), "rcbf_aql_run")
        if self.trajectory is not None and copy_back:
            o = self._keep[2]
            for f, t in self.trajectory.items():
                if f == "term_obs":
                    continue  # a side output: no buffer of the env or the outputs dict corresponds to it
                dst = self._env.obs if f == "obs" else o.get(f)
                if dst is not None and not (f == "goal_met" and self._env.dynamics_mode == "SimulatedCars"):
                    dst.copy_(t[self.K - 1])
        return self._env.obs, self._keep[2]["reward"], self._keep[2]["done"], self._keep[2]

    @property
    def dispatches(self):
        """Dispatch packets per run: K in the per-step form, one per 4096 steps in the fused form."""
        if not self._fin.alive:
            raise RuntimeError("the AQL plan was freed")
        return int(_lib.load().rcbf_aql_plan_dispatches(self._h))  # the handle is live: a count, never an error

    @property
    def form(self):
        """The kernel the plan's step packets dispatch: "per_step" (k_safe_step), "fused" (k_safe_steps and its
        trajectory forms) or "fused_fast" (k_safe_steps_fast, the cars fused plan's straight-line loop)."""
        if not self._fin.alive:
            raise RuntimeError("the AQL plan was freed")
        return FORMS[int(_lib.load().rcbf_aql_plan_form(self._h))]

    def times_ns(self):
        """(K, 2) int64 numpy array: each dispatch's start and end (ns, HSA
        system clock) from the last run; profiled plans only.  PROFILE_ENDS:
        the first dispatch's times in row 0, the last one's in row K - 1 (the
        same dispatch when the plan has one), 0 between."""
        import numpy as np
        if not self._fin.alive or not self.queue._fin.alive:
            raise RuntimeError("the AQL plan (or its queue) was freed")
        out = np.zeros((self.K, 2), dtype=np.uint64)
        _check(_lib.load().rcbf_aql_plan_times(self._h, out.ctypes.data), "rcbf_aql_plan_times")
        return out.astype(np.int64)

    def free(self):
        self._fin()


class ClosedLoopPlan(AqlPlan):
    """K closed-loop steps, policy and safe step alternating (see
    AqlQueue.closed_loop_plan).  `u_rl`: the plan's (B, n_u) action buffer."""

    def __init__(self, queue, handle, K, keep, env, trajectory, policy, u_rl, word):
        super().__init__(queue, handle, K, keep, False, env, trajectory)
        self.policy, self.u_rl, self._word = policy, u_rl, word

    @property
    def sampling(self):
        return self._word is not None

    def run(self, counter=None, sync_hip=True, timeout_us=0, copy_back=True):
        """AqlPlan.run.  A sampling plan's K steps draw with the counters
        c, c + 1, ..., c + K - 1: c = `counter`, or, when that is None,
        policy._counter, which then advances by K -- plans and policy.act()
        calls interleave without repeating a draw.  c is written to the
        plan's device word on the current stream, and the stream is
        synchronised before the doorbell (with sync_hip=False too, which skips
        only the device-wide synchronise), so packet 0 finds it there.  When
        obs is recorded, row K - 1 always goes back to env.obs, copy_back=False
        included: the next run's first packet reads env.obs."""
        dev = self.queue.device
        if self._word is not None:
            c = self.policy._counter if counter is None else int(counter)
            if counter is None:
                self.policy._counter += self.K
            c &= 0xFFFFFFFFFFFFFFFF
            with torch.cuda.device(dev):
                self._word.fill_(c - (1 << 64) if c >= 1 << 63 else c)
        elif counter is not None:
            raise ValueError("counter is the sampling plans' draw counter: this plan was built with evaluate=True")
        if not sync_hip:
            # the word's fill and the last run's copy into env.obs are on the current stream
            torch.cuda.current_stream(dev).synchronize()
        out = super().run(sync_hip=sync_hip, timeout_us=timeout_us, copy_back=copy_back)
        if self.trajectory is not None and not copy_back and "obs" in self.trajectory:
            self._env.obs.copy_(self.trajectory["obs"][self.K - 1])
        return out
