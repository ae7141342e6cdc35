"""Closed-loop evaluation of a policy on a batched env, all on the device.

The batched form of the reference's test loop (main.py:146-177; the same loop
in rcbf_sac/evaluator.py:20-54): reset, then per step
agent.select_action(obs, evaluate=True) -> env.step, summing reward and cost
until the episode ends, and the averages over the episodes.  Here the B envs
of a Batched*Env are the episodes: DevicePolicy.act (one launch) feeds
env.safe_step (one launch), EpisodeStats keeps the sums, and the host reads
once, after the last step.  With an AqlQueue the steps run as closed-loop AQL
plans instead (AqlQueue.closed_loop_plan: the policy's packet before every
step's, one doorbell per chunk of steps) and the host reads once per chunk.
"""
import numpy as np
import torch

from .episode_stats import EpisodeStats


def evaluate_policy(env, policy, layer, steps=None, mean=None, sigma=None, evaluate=True, queue=None, chunk=None):
    """Run `steps` (default env.max_episode_steps) closed-loop steps of
    policy.act(env.obs) -> env.safe_step(u, layer, mean, sigma) from a reset and
    return, over each env's FIRST finished episode,
      {"avg_reward", "avg_cost": means over those episodes (nan if none),
       "episodes": how many envs finished one,
       "reward", "cost": (B,) float64 (nan where none finished), "length": (B,) int32 (0 there)}.
    Envs auto-reset and keep stepping; their later episodes are not counted.
    No host synchronisation inside the loop: one read at the end, then
    env.check_failures().  A step is the two kernels, the three launches of
    EpisodeStats.update and nine small torch launches that keep each env's
    first record.
    queue: an AqlQueue on the env's device.  The steps then run as closed-loop
    AQL plans (AqlQueue.closed_loop_plan) of `chunk` steps (default
    min(steps, 256); the last one shorter when chunk does not divide steps)
    that record reward, cost and done: one doorbell and one
    EpisodeStats.update per chunk, each env's first record picked on the host.
    The same dict, bit for bit."""
    steps = int(env.max_episode_steps if steps is None else steps)
    if steps <= 0:
        raise ValueError(f"steps must be positive, got {steps}")
    if not hasattr(policy, "act"):
        raise ValueError("policy must be a DevicePolicy (or offer its act())")
    if (policy.n_o, policy.n_u) != (env.n_o, env.n_u):
        raise ValueError(f"the policy maps {policy.n_o} observations to {policy.n_u} actions, the env has "
                         f"{env.n_o} and {env.n_u}")
    if not evaluate and not getattr(policy, "has_log_std", True):
        raise NotImplementedError("evaluate=False needs a policy with a log-std head")
    dev = env.obs.device
    if policy.device != dev:
        raise ValueError(f"the policy is on {policy.device}, the env on {dev}")
    if dev.type != "cuda":
        raise ValueError("evaluate_policy needs a device env")
    if queue is not None:
        if chunk is not None and int(chunk) <= 0:
            raise ValueError(f"chunk must be positive, got {chunk}")
        env.reset()
        return _evaluate_plans(env, policy, layer, steps, mean, sigma, evaluate, queue, chunk)
    if chunk is not None:
        raise ValueError("chunk is the plan length of the queue path: pass queue as well")
    env.reset()
    return _evaluate_from(env, policy, layer, steps, mean, sigma, evaluate)


def _evaluate_plans(env, policy, layer, steps, mean=None, sigma=None, evaluate=True, queue=None, chunk=None):
    """evaluate_policy's loop from the env's current state as closed-loop
    plans (arguments already checked).  The episode sums carry from one
    update to the next, so the records are those of the per-step loop."""
    B = int(env.num_envs)
    chunk = min(steps, 256 if chunk is None else int(chunk))
    stats = EpisodeStats(env)  # lengths start from env.step_count
    o = env.make_outputs()
    traj = env.make_trajectory(chunk, ("reward", "cost", "done"))
    full, rest = divmod(steps, chunk)
    kw = dict(evaluate=evaluate, mean=mean, sigma=sigma, outputs=o)
    plans = [(queue.closed_loop_plan(env, policy, layer, chunk, trajectory=traj, **kw), full)]
    if rest:
        plans.append((queue.closed_loop_plan(env, policy, layer, rest,
                                             trajectory={f: t[:rest] for f, t in traj.items()}, **kw), 1))
    reward, cost = np.full(B, np.nan), np.full(B, np.nan)
    length, have = np.zeros(B, np.int32), np.zeros(B, bool)
    try:
        for plan, runs in plans:
            for _ in range(runs):
                plan.run()
                rec = stats.update(plan.trajectory, rows=plan.K)  # exact: an env may finish several episodes
                e = rec["env"].cpu().numpy()
                r, c, n = rec["reward"].cpu().numpy(), rec["cost"].cpu().numpy(), rec["length"].cpu().numpy()
                # the records come in step order: the first row of an env without a record yet is its first
                idx = np.unique(e, return_index=True)[1]
                idx = idx[~have[e[idx]]]
                reward[e[idx]], cost[e[idx]], length[e[idx]] = r[idx], c[idx], n[idx]
                have[e[idx]] = True
    finally:
        for plan, _ in plans:
            plan.free()
    n = int(have.sum())
    out = {"avg_reward": float(reward[have].mean()) if n else float("nan"),
           "avg_cost": float(cost[have].mean()) if n else float("nan"),
           "episodes": n, "reward": reward, "cost": cost, "length": length}
    env.check_failures()
    return out


def _evaluate_from(env, policy, layer, steps, mean=None, sigma=None, evaluate=True):
    """evaluate_policy's loop from the env's current state (arguments already
    checked): the open episodes count from their current step, their sums from
    zero."""
    B, dev = int(env.num_envs), env.obs.device
    stats = EpisodeStats(env)  # lengths start from env.step_count
    o = env.make_outputs()
    u = torch.empty(B, env.n_u, dtype=torch.float32, device=dev)
    traj = {"reward": o["reward"][None], "cost": o["cost"][None], "done": o["done"][None]}
    # each env's first record, column B the dump of every row that is none: rows [reward, cost, length, have]
    first = torch.full((4, B + 1), float("nan"), dtype=torch.float64, device=dev)
    first[2:].zero_()
    rows = torch.arange(B, device=dev)
    one = torch.ones(B, dtype=torch.float64, device=dev)
    for _ in range(steps):
        policy.act(env.obs, evaluate=evaluate, out=u)
        env.safe_step(u, layer, mean=mean, sigma=sigma, outputs=o)
        rec = stats.update(traj, max_episodes=B)  # at most one episode per env ends in a step
        e = rec["env"].long().clamp_(0, B - 1)    # rows past the count are uninitialised
        new = (rows < rec["count"][1]) & (first[3, e] == 0)
        slot = torch.where(new, e, B)
        first.scatter_(1, slot.expand(4, B), torch.stack((rec["reward"], rec["cost"], rec["length"], one)))
    host = first[:, :B].cpu().numpy()  # the one read
    have = host[3] != 0
    n = int(have.sum())
    out = {"avg_reward": float(host[0][have].mean()) if n else float("nan"),
           "avg_cost": float(host[1][have].mean()) if n else float("nan"),
           "episodes": n, "reward": host[0].copy(), "cost": host[1].copy(), "length": host[2].astype(np.int32)}
    env.check_failures()
    return out
