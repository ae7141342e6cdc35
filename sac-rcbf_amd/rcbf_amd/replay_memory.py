"""Device-resident ReplayMemory (rcbf_sac/replay_memory.py:5-38, SURVEY 8f
row 4).

The reference keeps a Python list of tuples, pushes in a Python loop
(batch_push, "TODO: Optimize This", :23-29) and samples with random.sample +
np.stack (:31-35).  Here the transitions live in HBM as one ring of packed
fp64 records [state | action | reward | next_state | mask | t | next_t]:
batch_push is one scatter launch (rcbf_ring_scatter_f64) and sample one
gather launch (rcbf_gather_rows_f64) on indices drawn without replacement
(uniform, like random.sample; numpy's Generator instead of Python's random,
so the sampled indices differ from the reference's stream).

sample() returns numpy arrays like the reference (mask as float64, t/next_t
NaN when they were pushed as None); sample_tensors() keeps them on the device
for the SAC update.

push_trajectory() takes the arrays of a K-step trajectory plan (rcbf_amd.aql)
and writes their K x B transitions into the ring in one launch
(rcbf_traj_pack_replay_f64): what the warm-up loop's memory.push per step
(main.py:100-107) leaves, terminal observations included.
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib


def check_trajectory(who, env, traj, needed, obs0, step0, rows, device):
    """The argument checks of a consumer of a trajectory plan's arrays
    (`who`: ReplayMemory.push_trajectory, DynamicsModel.trajectory_rows), made
    before any library call: the `needed` fields and, when present, "term_obs"
    are tensors of the dtype and shape env._trajectory_spec() gives, on
    `device`, [:, :B] views of dense (K, P[, w]) arrays of one pitch P with at
    least `rows` rows; obs0 (B, n_o) f32 and step0 (B,) i32 contiguous on
    `device`.  Returns ({field: tensor}, K, pitch); raises ValueError."""
    B, n_o = env.num_envs, env.n_o
    for f in needed:
        if f not in traj:
            raise ValueError(f"{who} needs trajectory[{f!r}]")
    spec = env._trajectory_spec()
    fields = {f: traj[f] for f in (*needed, "term_obs") if traj.get(f) is not None}
    K = min(int(t.shape[0]) for t in fields.values()) if rows is None else int(rows)
    pitch = None
    for f, t in fields.items():
        w, dt = spec[f]
        want = (B, w) if w else (B,)
        if not (torch.is_tensor(t) and t.dtype == dt and t.device == device and t.dim() == len(want) + 1
                and tuple(t.shape[1:]) == want):
            raise ValueError(f"trajectory[{f!r}] must be a {dt} tensor of shape (K, {', '.join(map(str, want))}) "
                             f"on {device}")
        ww = w or 1
        st = t.stride()
        if st[1:] != ((w, 1) if w else (1,)) or st[0] % ww or st[0] // ww < B:
            raise ValueError(f"trajectory[{f!r}] must be a [:, :B] view of a dense (K, P{', w' if w else ''}) "
                             f"array (use env.make_trajectory), got strides {st}")
        if pitch is not None and st[0] // ww != pitch:
            raise ValueError(f"trajectory[{f!r}] has row pitch {st[0] // ww}, the other fields {pitch}")
        pitch = st[0] // ww
        if t.shape[0] < K:
            raise ValueError(f"trajectory[{f!r}] has {t.shape[0]} rows, rows = {K}")
    if K <= 0:
        raise ValueError(f"rows must be positive, got {K}")
    if not (torch.is_tensor(obs0) and obs0.dtype == torch.float32 and obs0.device == device
            and tuple(obs0.shape) == (B, n_o) and obs0.is_contiguous()):
        raise ValueError(f"obs0 must be a contiguous float32 tensor of shape ({B}, {n_o}) on {device}")
    if not (torch.is_tensor(step0) and step0.dtype == torch.int32 and step0.device == device
            and tuple(step0.shape) == (B,) and step0.is_contiguous()):
        raise ValueError(f"step0 must be a contiguous int32 tensor of shape ({B},) on {device}")
    return fields, K, pitch


class ReplayMemory:

    def __init__(self, capacity, seed, device=None):
        self.capacity = int(capacity)
        self.position = 0
        self._size = 0
        self._rng = np.random.default_rng(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._ring = None
        self._dims = None  # (n_s, n_u)

    # -- layout -------------------------------------------------------------
    def _width(self):
        n_s, n_u = self._dims
        return 2 * n_s + n_u + 4

    def _pack(self, state, action, reward, next_state, mask, t, next_t):
        def col(v, n):
            if v is None:
                return torch.full((n, 1), float("nan"), dtype=torch.float64, device=self.device)
            v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
            return v.to(device=self.device, dtype=torch.float64).reshape(n, -1)

        state = state if torch.is_tensor(state) else np.asarray(state, dtype=np.float64)
        n = state.shape[0]
        st = col(state, n)
        act = col(action, n)
        if self._dims is None:
            self._dims = (st.shape[1], act.shape[1])
            self._ring = torch.empty(self.capacity, self._width(), dtype=torch.float64, device=self.device)
        if (st.shape[1], act.shape[1]) != self._dims:
            raise ValueError(f"transition shapes {(st.shape[1], act.shape[1])} != {self._dims}")
        rec = torch.cat([st, act, col(reward, n), col(next_state, n), col(mask, n), col(t, n), col(next_t, n)], 1)
        return rec.contiguous()

    # -- reference API ------------------------------------------------------
    def push(self, state, action, reward, next_state, mask, t=None, next_t=None):
        def one(v):
            return None if v is None else (v.unsqueeze(0) if torch.is_tensor(v) else np.asarray(v)[None])
        self.batch_push(one(state), one(action), one(reward), one(next_state), one(mask), one(t), one(next_t))

    def batch_push(self, state_batch, action_batch, reward_batch, next_state_batch, mask_batch, t_batch=None,
                   next_t_batch=None):
        if t_batch is None or next_t_batch is None:  # the reference drops both unless both are given (:25-29)
            t_batch = next_t_batch = None
        rec = self._pack(state_batch, action_batch, reward_batch, next_state_batch, mask_batch, t_batch,
                         next_t_batch)
        n = rec.shape[0]
        if n == 0:
            return
        if n > self.capacity:  # the sequential pushes leave only the last `capacity` records
            self.position = (self.position + n - self.capacity) % self.capacity
            rec = rec[n - self.capacity:].contiguous()
            n = self.capacity
        rc = _lib.load().rcbf_ring_scatter_f64(_lib.ptr(self._ring), self.capacity, rec.shape[1], self.position,
                                               _lib.ptr(rec), n, _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_ring_scatter_f64")
        self.position = (self.position + n) % self.capacity
        self._size = min(self._size + n, self.capacity)

    def push_trajectory(self, env, traj, obs0, step0, rows=None, auto_reset=True):
        """The `rows` (default: all) steps of a trajectory plan of `env`
        (AqlQueue.safe_step_plan(trajectory=traj)) as rows x B transitions, in
        the order B envs stepped in lock-step would push them (step-major):
        one rcbf_traj_pack_replay_f64 launch, no intermediate tensor.
        obs0 (B, n_o) f32: the observation step 0 acted on (env.obs before the
        run, cloned); step0 (B,) i32: env.step_count before the run, cloned.
        traj needs "obs", "u", "reward", "done"; with "term_obs" (and
        auto_reset, as the plan ran) the next_obs of a transition that ended
        an episode is the terminal observation, without it the next episode's
        first (warned about once).  mask, t and next_t follow main.py:100-107:
        mask 1 at the time limit, else 1 - done; t the episode step x dt."""
        B, n_o, n_u = env.num_envs, env.n_o, env.n_u
        fields, K, pitch = check_trajectory("push_trajectory", env, traj, ("obs", "u", "reward", "done"), obs0, step0,
                                            rows, self.device)
        term = fields.get("term_obs")
        if term is None and auto_reset and not getattr(self, "_warned_no_term_obs", False):
            self._warned_no_term_obs = True
            warnings.warn("push_trajectory without trajectory['term_obs']: the next_obs of a transition that ends an "
                          "episode is the next episode's first observation (record term_obs with the plan)")
        if self._dims is None:
            self._dims = (n_o, n_u)
            self._ring = torch.empty(self.capacity, self._width(), dtype=torch.float64, device=self.device)
        if (n_o, n_u) != self._dims:
            raise ValueError(f"transition shapes {(n_o, n_u)} != {self._dims}")
        rc = _lib.load().rcbf_traj_pack_replay_f64(
            _lib.ptr(self._ring), self.capacity, self.position, B, K, pitch, n_o, n_u, _lib.ptr(obs0),
            _lib.ptr(step0), _lib.ptr(fields["obs"]), _lib.ptr(term), _lib.ptr(fields["u"]),
            _lib.ptr(fields["reward"]), _lib.ptr(fields["done"]), int(env.max_episode_steps), float(env.dt),
            int(bool(auto_reset)), _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_traj_pack_replay_f64")
        n = K * B
        self.position = (self.position + n) % self.capacity
        self._size = min(self._size + n, self.capacity)

    def sample_tensors(self, batch_size):
        """(state, action, reward, next_state, mask, t, next_t) device tensors."""
        if batch_size > self._size or batch_size < 0:
            raise ValueError("Sample larger than population or is negative")
        idx = torch.as_tensor(self._rng.choice(self._size, batch_size, replace=False).astype(np.int64),
                              device=self.device)
        out = torch.empty(batch_size, self._width(), dtype=torch.float64, device=self.device)
        rc = _lib.load().rcbf_gather_rows_f64(_lib.ptr(out), _lib.ptr(self._ring), out.shape[1], _lib.ptr(idx),
                                              batch_size, _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_gather_rows_f64")
        n_s, n_u = self._dims
        o = 0
        parts = []
        for w in (n_s, n_u, 1, n_s, 1, 1, 1):
            parts.append(out[:, o:o + w])
            o += w
        s, a, r, ns, m, t, nt = parts
        return s, a, r[:, 0], ns, m[:, 0], t[:, 0], nt[:, 0]

    def sample(self, batch_size):
        return tuple(v.cpu().numpy() for v in self.sample_tensors(batch_size))

    def __len__(self):
        return self._size
