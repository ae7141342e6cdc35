"""Per-episode return, cost and length of a batched env, kept on the device.

The reference's loops keep three Python scalars per episode --
episode_reward += reward, episode_cost += info['cost'], episode_steps += 1
(main.py:98-101) -- and log them when the episode ends (main.py:140-144; the
same again in main.py:152-170 and rcbf_sac/evaluator.py:33-54).  EpisodeStats
does that bookkeeping for the B envs of a Batched*Env over the (K, B) reward,
cost and done arrays of a trajectory plan (AqlQueue.safe_step_plan(
trajectory=...)) in one library call (rcbf_traj_episode_stats_f64: count, scan,
pack), the third consumer of a plan beside ReplayMemory.push_trajectory and
DynamicsModel.append_trajectory.  The running sums of the episodes still open
at the end of one plan carry into the next update, so a run cut into plans
gives the records of the uncut run, bit for bit.

All sums are fp64 over the fp32 values, added in step order: the records are
bit-reproducible from the arrays.  (The reference's accumulator has whatever
dtype numpy's promotion gives `0 + reward`; that is not reproduced)
"""
import torch

from . import _lib

_FIELDS = {"reward": torch.float32, "cost": torch.float32, "done": torch.uint8}


def check_stats_trajectory(B, traj, rows, device):
    """update()'s argument checks, made before any library call (in the style
    of replay_memory.check_trajectory, which also wants obs0 and step0):
    "reward", "done" and, when present, "cost" are [:, :B] views of dense
    (K, P) arrays of one pitch P, of the right dtypes, on `device`, with at
    least `rows` rows.  Returns ({field: tensor}, K, pitch); raises ValueError."""
    for f in ("reward", "done"):
        if traj.get(f) is None:
            raise ValueError(f"EpisodeStats.update needs trajectory[{f!r}]")
    fields = {f: traj[f] for f in _FIELDS if traj.get(f) is not None}
    for f, t in fields.items():
        if not (torch.is_tensor(t) and t.dtype == _FIELDS[f] and t.device == device and t.dim() == 2
                and t.shape[1] == B):
            raise ValueError(f"trajectory[{f!r}] must be a {_FIELDS[f]} tensor of shape (K, {B}) on {device}")
    K = min(int(t.shape[0]) for t in fields.values()) if rows is None else int(rows)
    if K <= 0:
        raise ValueError(f"rows must be positive, got {K}")
    pitch = None
    for f, t in fields.items():
        st = t.stride()
        if st[1] != 1 or st[0] < B:
            raise ValueError(f"trajectory[{f!r}] must be a [:, :B] view of a dense (K, P) array (use "
                             f"env.make_trajectory), got strides {st}")
        if pitch is not None and st[0] != pitch:
            raise ValueError(f"trajectory[{f!r}] has row pitch {st[0]}, the other fields {pitch}")
        pitch = st[0]
        if t.shape[0] < K:
            raise ValueError(f"trajectory[{f!r}] has {t.shape[0]} rows, rows = {K}")
    return fields, K, pitch


class EpisodeRecords(dict):
    """update()'s result: "env", "step", "length" (int32) and "reward", "cost"
    (float64) device tensors, one row per finished episode in the order B envs
    stepped in lock-step would log them; "count", the device int64 pair
    {episodes finished, rows written}; and "n_episodes", the first of the two
    as an int.  After update(max_episodes=n) nothing has been read from the
    device: the five arrays have n rows, and looking at "n_episodes" makes the
    one 16-byte read and trims them to the rows written."""

    ARRAYS = ("env", "step", "length", "reward", "cost")

    def __missing__(self, key):
        if key != "n_episodes":
            raise KeyError(key)
        n_ep, n = (int(v) for v in self["count"].tolist())
        for f in self.ARRAYS:
            self[f] = self[f][:n]
        self[key] = n_ep
        return n_ep


class EpisodeStats:

    def __init__(self, env, device=None):
        self.env = env
        self.num_envs = int(env.num_envs)
        self.device = torch.device(device) if device is not None else env.step_count.device
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # (return, cost) and the episode-step count of every env's open episode: in and out of a call are
        # separate arrays (ping-pong), so no lane reads what another call's lane writes
        self._carry = torch.zeros(2, self.num_envs, 2, dtype=torch.float64, device=self.device)
        self._len = torch.zeros(2, self.num_envs, dtype=torch.int32, device=self.device)
        self._len[0].copy_(env.step_count)
        self._cur = 0
        self._scratch = None

    def reset(self):
        """Every env at the start of an episode: zero sums, zero lengths."""
        self._carry.zero_()
        self._len.zero_()

    def running(self):
        """((B, 2) f64 [return, cost], (B,) i32 length) of the open episodes."""
        return self._carry[self._cur], self._len[self._cur]

    def _call(self, lib, rec_i, rec_f, count, K, pitch, fields, advance, auto_reset, max_rows):
        B, dev, a, b = self.num_envs, self.device, self._cur, 1 - self._cur
        words = lib.rcbf_traj_episode_stats_scratch_bytes(B, K) // 8
        if self._scratch is None or self._scratch.numel() < words:
            self._scratch = torch.empty(words, dtype=torch.int64, device=dev)
        rows = [None] * 5 if max_rows == 0 else [rec_i[0], rec_i[1], rec_i[2], rec_f[0], rec_f[1]]
        state = [self._carry[a], self._len[a], self._carry[b], self._len[b]] if advance else [None] * 4
        with torch.cuda.device(dev):
            rc = lib.rcbf_traj_episode_stats_f64(
                *(_lib.ptr(t) for t in rows), _lib.ptr(count), _lib.ptr(self._scratch), B, K, pitch,
                _lib.ptr(fields["reward"]), _lib.ptr(fields.get("cost")), _lib.ptr(fields["done"]),
                *(_lib.ptr(t) for t in state), int(bool(auto_reset)), max_rows, _lib.stream_of(dev))
        _lib.check(rc, "rcbf_traj_episode_stats_f64")
        if advance:
            self._cur = b

    def update(self, traj, rows=None, auto_reset=True, max_episodes=None):
        """Account the `rows` (default: all) steps of a trajectory: per env and
        step, return += reward, cost += cost (if the trajectory has "cost"),
        length += 1; where done is set (and auto_reset, as the plan ran) the
        episode is recorded and the three start again from zero.  Returns
        EpisodeRecords.
        max_episodes=None: exact -- a count-only call, one 8-byte read of the
        number of episodes, then the call that writes them.  An int: one call
        into arrays of that many rows, the first max_episodes episodes kept,
        nothing read from the device until "n_episodes" is looked at.
        The output buffers of ONE safe_step viewed as one-row arrays are a
        valid trajectory: {"reward": out["reward"][None], ...}."""
        B, dev = self.num_envs, self.device
        fields, K, pitch = check_stats_trajectory(B, traj, rows, dev)
        if max_episodes is not None and int(max_episodes) < 0:
            raise ValueError(f"max_episodes must not be negative, got {max_episodes}")
        if B == 0:  # no env, no episode: no launch
            rec_i = torch.empty(3, 0, dtype=torch.int32, device=dev)
            rec_f = torch.empty(2, 0, dtype=torch.float64, device=dev)
            return EpisodeRecords(zip(EpisodeRecords.ARRAYS, (*rec_i, *rec_f)), n_episodes=0,
                                  count=torch.zeros(2, dtype=torch.int64, device=dev))
        if dev.type != "cuda":
            raise ValueError("EpisodeStats.update needs HIP device tensors")
        lib = _lib.load()
        count = torch.empty(2, dtype=torch.int64, device=dev)
        exact = max_episodes is None
        if exact:  # how many end: nothing is advanced
            self._call(lib, None, None, count, K, pitch, fields, False, auto_reset, 0)
            n = int(count[0].item())
        else:
            n = int(max_episodes)
        rec_i = torch.empty(3, n, dtype=torch.int32, device=dev)
        rec_f = torch.empty(2, n, dtype=torch.float64, device=dev)
        self._call(lib, rec_i, rec_f, count, K, pitch, fields, True, auto_reset, n)
        out = EpisodeRecords(zip(EpisodeRecords.ARRAYS, (*rec_i, *rec_f)), count=count)
        if exact:
            out["n_episodes"] = n
        return out
