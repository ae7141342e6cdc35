"""What the terminal observation and the replay packing cost: one process, one
arm; prints one JSON line per measurement.  Driven by a job that alternates the
arms, several processes a side, each under `timeout`.

  --what plan --form traj|term   the fused trajectory plan (every field of
        TRAJECTORY_FIELDS recorded; k_safe_steps_traj, the same machine code as
        before term_obs existed) against the same plan with term_obs
        (k_safe_steps_term): median host time of plan.run(sync_hip=False,
        copy_back=False) per step, K = 20 and 1 000, bench.py's start states
        and action pool.
  --what pack                    ReplayMemory.push_trajectory (one
        rcbf_traj_pack_replay_f64 launch) of a K = 20 trajectory against the
        torch assembly of the same records followed by batch_push, device time
        between two events, median over the repetitions; the algorithmic bytes
        (read: obs, u, reward, done; written: the records) over the time.
B = 65 536."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sac-rcbf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_env(name, B, dev):
    import torch

    import bench
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv

    class Args:
        cuda = True

    if name == "cars":
        env, mode = BatchedSimulatedCarsEnv(B, device=dev, seed=1234), "SimulatedCars"
    else:
        env, mode = BatchedUnicycleEnv(B, device=dev, seed=1234, hazards_locations=bench.unicycle_hazards(5)), "Unicycle"
    layer = CBFQPLayer(env, Args(), gamma_b=20.0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    bench.init_states(env, gen, mode)
    pool = [(torch.rand(B, env.n_u, device="cuda", generator=gen) * 2 - 1).contiguous() for _ in range(7)]
    return env, layer, pool


def plan_arm(a):
    import torch

    from rcbf_amd.aql import AqlQueue
    dev = torch.device("cuda", 0)
    q = AqlQueue(dev)
    for K, reps in ((20, 3000), (1000, 100)):
        env, layer, pool = make_env(a.env, a.batch, dev)
        fields = env.TRAJECTORY_FIELDS + (("term_obs",) if a.form == "term" else ())
        traj = env.make_trajectory(K, fields)
        plan = q.safe_step_plan(env, pool, layer, steps=K, outputs=env.make_outputs(), trajectory=traj)
        torch.cuda.synchronize()
        for _ in range(max(3, reps // 20)):
            plan.run(sync_hip=False, copy_back=False)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter_ns()
            plan.run(sync_hip=False, copy_back=False)
            ts.append(time.perf_counter_ns() - t0)
        ts.sort()
        env.check_failures()
        print(json.dumps({"what": "plan", "form": a.form, "env": a.env, "K": K, "B": a.batch,
                          "dispatches": plan.dispatches, "reps": reps,
                          "us_per_step_median": round(ts[len(ts) // 2] / 1e3 / K, 4),
                          "us_per_step_p10": round(ts[len(ts) // 10] / 1e3 / K, 4),
                          "us_per_step_p90": round(ts[9 * len(ts) // 10] / 1e3 / K, 4)}), flush=True)
        plan.free()
        del plan, env, layer, traj
    q.close()


def assemble(env, traj, obs0, step0, K):
    """The records' fields with torch, by the rules of include/rcbf_hip.h: the only way before push_trajectory."""
    import torch
    B = env.num_envs
    obs, done = traj["obs"][:K], traj["done"][:K] != 0
    prev = torch.cat([obs0[None], obs[:-1]], 0)
    nxt = torch.where(done[..., None], traj["term_obs"][:K], obs)
    e = torch.empty(K, B, dtype=torch.int64, device=obs.device)
    c = step0.to(torch.int64)
    for j in range(K):
        e[j] = c + 1
        c = torch.where(done[j], torch.zeros_like(c), e[j])
    mask = torch.where(e == env.max_episode_steps, 1.0, 1.0 - done.to(torch.float64))
    t, nt = e.to(torch.float64) * env.dt, (e + 1).to(torch.float64) * env.dt
    n = K * B
    return (prev.reshape(n, -1), traj["u"][:K].reshape(n, -1), traj["reward"][:K].reshape(n), nxt.reshape(n, -1),
            mask.reshape(n), t.reshape(n), nt.reshape(n))


def pack_arm(a):
    import torch

    from rcbf_amd.replay_memory import ReplayMemory
    dev = torch.device("cuda", 0)
    K, B = 20, a.batch
    env, layer, pool = make_env(a.env, B, dev)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    traj = env.make_trajectory(K, ("obs", "u", "reward", "done", "term_obs"))
    for f, t in traj.items():
        if f == "done":
            t.copy_((torch.rand(K, B, device="cuda", generator=gen) < 1 / 300).to(torch.uint8))
        else:
            t.copy_(torch.randn(t.shape, device="cuda", generator=gen))
    obs0 = torch.randn(B, env.n_o, device="cuda", generator=gen)
    step0 = torch.randint(0, env.max_episode_steps - K, (B,), device="cuda", generator=gen, dtype=torch.int32)
    W = 2 * env.n_o + env.n_u + 4
    read = 4 * (env.n_o + env.n_u + 1) + 1
    out = {"what": "pack", "env": a.env, "K": K, "B": B, "bytes_read_per_transition": read,
           "bytes_written_per_transition": 8 * W}

    def timed(fn, reps):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        ts = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
        return ts[len(ts) // 2], ts[len(ts) // 10], ts[9 * len(ts) // 10]

    mem = ReplayMemory(3 * K * B + 11, 0, device=dev)
    med, p10, p90 = timed(lambda: mem.push_trajectory(env, traj, obs0, step0), 200)
    out.update({"pack_us_median": round(med, 2), "pack_us_p10": round(p10, 2), "pack_us_p90": round(p90, 2),
                "pack_TB_per_s": round(K * B * (read + 8 * W) / med / 1e6, 3)})
    twin = ReplayMemory(3 * K * B + 11, 0, device=dev)
    med, p10, p90 = timed(lambda: twin.batch_push(*assemble(env, traj, obs0, step0, K)), 30)
    out.update({"torch_us_median": round(med, 2), "torch_us_p10": round(p10, 2), "torch_us_p90": round(p90, 2),
                "torch_over_pack": round(med / out["pack_us_median"], 2)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=["plan", "pack"])
    ap.add_argument("--form", default="term", choices=["traj", "term"])
    ap.add_argument("--env", default="cars", choices=["cars", "u5"])
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    (plan_arm if a.what == "plan" else pack_arm)(a)


if __name__ == "__main__":
    main()
