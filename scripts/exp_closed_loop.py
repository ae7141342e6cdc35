"""What a closed-loop step -- the policy's forward, then the safe step it feeds
-- costs through three launch paths.  One process; prints one JSON line per
(env, B) and, with --out, writes all of them to one JSON file.

Legs, each over K = --steps closed-loop steps with evaluate=True and a
H = --hidden policy, on envs of the same seed:
  eager  the launch loop: policy.act(env.obs, out=u) then env.safe_step(u),
         K times on torch's stream (two HIP launches per step)
  graph  the same two launches captured once in a hipGraph, replayed K times
  plan   AqlQueue.closed_loop_plan of K steps (2K packets, one doorbell):
         wall clock around run(sync_hip=False) after a synchronise; and
         plan_dev, the device period of the same runs (first packet's start to
         last packet's end, PROFILE_ENDS) on a second plan on a profiling queue
Wall clock (perf_counter) around K steps that end in a synchronise (the plan's
run is synchronous), per step in us.  Each leg is warmed with one block of K
steps; then --rounds rounds, the legs alternating inside a round, --reps blocks
per leg and round.  Reported per leg: the median block, the 10th and 90th
percentile, min and max over rounds x reps blocks.  The envs keep stepping from
block to block (episodes end and reset inside the blocks, as in a rollout).

And, with --evaluate, the wall time of evaluate_policy(steps=300) at B = 4 096
on the cars env with and without queue=, alternating, the median of 5.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sac-rcbf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class Args:
    cuda = True


def make_policy(env, hidden, seed=11):
    """A GaussianPolicy-shaped module with small seeded weights (|mean| < 1: unsaturated actions)."""
    import torch
    from rcbf_amd.policy import DevicePolicy
    gen = torch.Generator().manual_seed(seed)

    def linear(n_in, n_out):
        m = torch.nn.Linear(n_in, n_out)
        with torch.no_grad():
            m.weight.copy_(torch.randn(n_out, n_in, generator=gen) * (0.5 / n_in ** 0.5))
            m.bias.copy_(torch.randn(n_out, generator=gen) * 0.1)
        return m

    mod = torch.nn.Module()
    mod.linear1, mod.linear2 = linear(env.n_o, hidden), linear(hidden, hidden)
    mod.mean_linear, mod.log_std_linear = linear(hidden, env.n_u), linear(hidden, env.n_u)
    mod.action_scale, mod.action_bias = torch.ones(env.n_u), torch.zeros(env.n_u)
    return DevicePolicy(mod.to(env.device), device=env.device)


def make_env(name, B, seed=3):
    import numpy as np
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv
    if name == "cars":
        env = BatchedSimulatedCarsEnv(B, seed=seed)
    else:
        env = BatchedUnicycleEnv(B, seed=seed, hazards_locations=np.array([[0., 0.], [-1., 1.], [-1., -1.]]) * 1.5)
    return env, CBFQPLayer(env, Args(), gamma_b=20.0)


def summary(us):
    s = sorted(us)
    n = len(s)
    return {"median_us": round(s[n // 2], 3), "p10_us": round(s[n // 10], 3), "p90_us": round(s[(9 * n) // 10], 3),
            "min_us": round(s[0], 3), "max_us": round(s[-1], 3), "blocks": n}


def measure(name, B, a):
    import torch
    from rcbf_amd.aql import PROFILE_ENDS, AqlQueue
    K = a.steps
    dev = torch.device("cuda", 0)
    envs = [make_env(name, B) for _ in range(4)]  # eager, graph, plan, profiled plan
    pol = make_policy(envs[0][0], a.hidden)
    outs = [e.make_outputs() for e, _ in envs]
    us = [torch.empty(B, e.n_u, dtype=torch.float32, device=dev) for e, _ in envs]

    def step(i):
        e, layer = envs[i]
        pol.act(e.obs, evaluate=True, out=us[i])
        e.safe_step(us[i], layer, outputs=outs[i])

    def eager():
        for _ in range(K):
            step(0)
        torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(1)  # warm-up on the side stream, before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(1)

    def replay():
        for _ in range(K):
            graph.replay()
        torch.cuda.synchronize()

    q, qp = AqlQueue(dev), AqlQueue(dev, profile=True)
    plan = q.closed_loop_plan(envs[2][0], pol, envs[2][1], K, evaluate=True, outputs=outs[2])
    prof = qp.closed_loop_plan(envs[3][0], pol, envs[3][1], K, evaluate=True, outputs=outs[3],
                               fence_flags=PROFILE_ENDS)
    assert plan.dispatches == 2 * K

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6 / K

    def device_period():
        torch.cuda.synchronize()
        prof.run(sync_hip=False)
        t = prof.times_ns()
        return float(t[K - 1, 1] - t[0, 0]) / 1e3 / K

    legs = {"eager": lambda: wall(eager), "graph": lambda: wall(replay),
            "plan": lambda: wall(lambda: plan.run(sync_hip=False)), "plan_dev": device_period}
    got = {k: [] for k in legs}
    for fn in legs.values():
        fn()  # warm every leg at this shape
    for _ in range(a.rounds):
        for k, fn in legs.items():
            got[k].extend(fn() for _ in range(a.reps))
    for e, _ in envs:
        e.check_failures()
    plan.free()
    prof.free()
    q.close()
    qp.close()
    out = {"env": name, "B": B, "K": K, "hidden": a.hidden, "evaluate": True, "rounds": a.rounds, "reps": a.reps,
           "unit": "us per closed-loop step (policy + safe step)", **{k: summary(v) for k, v in got.items()}}
    out["plan_over_graph"] = round(out["plan"]["median_us"] / out["graph"]["median_us"], 3)
    out["plan_over_eager"] = round(out["plan"]["median_us"] / out["eager"]["median_us"], 3)
    print(json.dumps(out), flush=True)
    return out


def measure_evaluate(a, B=4096, steps=300, reps=5):
    import torch
    from rcbf_amd.aql import AqlQueue
    from rcbf_amd.evaluator import evaluate_policy
    (e1, l1), (e2, l2) = make_env("cars", B), make_env("cars", B)
    pol = make_policy(e1, a.hidden)
    q = AqlQueue(torch.device("cuda", 0))
    t = {"launch_loop": [], "queue": []}
    res = {}
    for r in range(reps + 1):  # the first pass warms both
        for k, fn in (("launch_loop", lambda: evaluate_policy(e1, pol, l1, steps=steps)),
                      ("queue", lambda: evaluate_policy(e2, pol, l2, steps=steps, queue=q))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            if r:
                t[k].append((time.perf_counter() - t0) * 1e3)
    same = all(res["queue"][f].tobytes() == res["launch_loop"][f].tobytes() for f in ("reward", "cost", "length"))
    q.close()
    out = {"what": "evaluate_policy wall time", "env": "cars", "B": B, "steps": steps, "hidden": a.hidden,
           "episodes": res["queue"]["episodes"], "results_bit_equal": bool(same),
           **{k + "_ms": {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3),
                          "max": round(max(v), 3), "reps": len(v)} for k, v in t.items()}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="cars,unicycle")
    ap.add_argument("--batches", default="256,4096,65536")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "exp_closed_loop.py measures on the GPU"
    rows = [measure(name, int(B), a) for name in a.envs.split(",") for B in a.batches.split(",")]
    doc = {"device": torch.cuda.get_device_name(0), "steps": rows}
    if a.evaluate:
        doc["evaluate_policy"] = measure_evaluate(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
