"""The reference loop's episode bookkeeping over (K, B) arrays, restated in
numpy as the oracle of rcbf_traj_episode_stats_f64: a literal per-env Python
loop of main.py:98-101 (episode_reward += reward; episode_cost +=
info['cost']; episode_steps += 1) and :140-144 (the episode that ends is
logged and the three start again), with np.float64 accumulators."""
import numpy as np

FIELDS = ("env", "step", "length", "reward", "cost")


def episode_loop(reward, cost, done, carry_in=None, len_in=None, auto_reset=True):
    """reward, cost [or None]: (K, B) float32; done (K, B) bool or uint8;
    carry_in [or None] (B, 2) float64; len_in [or None] (B,) int32.  Returns
    (records, carry (B, 2) float64, length (B,) int32): records a dict of the
    five arrays, step-major, env-minor -- the order in which B envs stepped in
    lock-step would log them."""
    K, B = reward.shape
    recs = []
    carry, length = np.zeros((B, 2), np.float64), np.zeros(B, np.int32)
    for i in range(B):
        R = np.float64(0.0 if carry_in is None else carry_in[i, 0])
        C = np.float64(0.0 if carry_in is None else carry_in[i, 1])
        c = 0 if len_in is None else int(len_in[i])
        for j in range(K):
            R = R + np.float64(reward[j, i])
            if cost is not None:
                C = C + np.float64(cost[j, i])
            e = c + 1
            if done[j, i] and auto_reset:
                recs.append((j, i, e, R, C))
                R, C, c = np.float64(0.0), np.float64(0.0), 0
            else:
                c = e
        carry[i] = (R, C)
        length[i] = c
    recs.sort(key=lambda r: (r[0], r[1]))
    out = {"step": np.array([r[0] for r in recs], np.int32), "env": np.array([r[1] for r in recs], np.int32),
           "length": np.array([r[2] for r in recs], np.int32), "reward": np.array([r[3] for r in recs], np.float64),
           "cost": np.array([r[4] for r in recs], np.float64)}
    return out, carry, length


def bits(a):
    """An array for np.array_equal: doubles as their int64 bit patterns."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_records(a, b):
    return all(np.array_equal(bits(a[f]), bits(b[f])) for f in FIELDS)


def synthetic(K, B, seed, p_done=0.3):
    """reward, cost: randn * exp(4 randn) in fp32 (magnitudes over many
    binades, so the order of the additions shows in the bits); done with
    p = p_done; random carry_in and len_in."""
    rng = np.random.default_rng(seed)

    def wide(*shape):
        return (rng.standard_normal(shape) * np.exp(4.0 * rng.standard_normal(shape))).astype(np.float32)

    return {"reward": wide(K, B), "cost": wide(K, B), "done": (rng.random((K, B)) < p_done).astype(np.uint8),
            "carry": wide(B, 2).astype(np.float64) * 1.000000123, "len": rng.integers(0, 300, B).astype(np.int32)}
