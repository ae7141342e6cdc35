"""What DynamicsModel.trajectory_rows (rcbf_traj_pack_gp_f64: count, scan, pack)
costs, against the two ways there were before it.  One process; prints one JSON
line per (env, shape, keep_last) and, with --out, appends them to a file.

Arms, on the same synthetic trajectory (random fp32 rows, done with p = 1/300,
random step0, so most waves hold selected and unselected lanes at every step):
  rows    dm.trajectory_rows(every=2, keep_last=...): the three launches, the
          output allocation and the 16-byte read of the row count
  launch  rcbf_traj_pack_gp_f64 alone into preallocated arrays (no host read):
          the device time the algorithmic bytes are divided by
  torch   (a) the same rows assembled with torch ops on the device: the episode
          steps by a K-step loop, a boolean mask's nonzero for the compaction,
          gathers, fp64 get_state and the rate of DynamicsModel._f_plus_gu
  host    (b) the Python loop over the steps on the host that was the only way:
          device -> host copies, numpy get_state, append_transition per step
          (fit_gp_model stubbed), wall clock, 3 repetitions
rows / launch / torch: device time between two events, warmed, the median of
--reps (>= 20) per round; --rounds (5) alternating rounds of rows and torch, so
"faster in each pair" is read off the per-round medians.
Algorithmic bytes: read 4 (n_o + n_u) + 1 per transition (cars 45), written
16 n_s per selected row (cars 160).  The repetitions reuse one set of inputs
and outputs, 164 MB at (65 536, 20) for cars, inside the 256 MB Infinity Cache:
the bytes/s are warm-cache figures, not cold-HBM ones.  The two device paths
are compared before anything is timed (asserted: equal states, d within 1e-12)."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sac-rcbf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIMS = {"cars": ("SimulatedCars", 10, 1, 10, 300), "unicycle": ("Unicycle", 7, 2, 3, 1000)}


class Env:
    """What trajectory_rows reads of an env."""

    def __init__(self, name, B):
        self.dynamics_mode, self.n_o, self.n_u, self.n_s, self.max_episode_steps = DIMS[name]
        self.num_envs, self.dt = B, 0.02

    def _trajectory_spec(self):
        import torch
        return {"obs": (self.n_o, torch.float32), "u": (self.n_u, torch.float32), "done": (0, torch.uint8),
                "term_obs": (self.n_o, torch.float32)}


def make_trajectory(env, K, gen):
    import torch
    B, P = env.num_envs, (env.num_envs + 63) // 64 * 64

    def r(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)

    traj = {"obs": r(K, P, env.n_o)[:, :B], "term_obs": r(K, P, env.n_o)[:, :B], "u": r(K, P, env.n_u)[:, :B],
            "done": (torch.rand(K, P, device="cuda", generator=gen) < 1 / 300).to(torch.uint8)[:, :B]}
    obs0 = r(B, env.n_o)
    step0 = torch.randint(0, env.max_episode_steps - 1, (B,), device="cuda", generator=gen, dtype=torch.int32)
    return traj, obs0, step0


def torch_rows(env, traj, obs0, step0, K, every, keep_last):
    """(a): the rows with torch ops on the device."""
    import torch
    B, dt = env.num_envs, env.dt
    obs, done = traj["obs"][:K], traj["done"][:K] != 0
    e = torch.empty(K, B, dtype=torch.int64, device=obs.device)
    c = step0.to(torch.int64)
    for j in range(K):
        e[j] = c + 1
        c = torch.where(done[j], torch.zeros_like(c), e[j])
    idx = (e % every == 0).reshape(-1).nonzero()[:, 0]  # step-major, env-minor
    n_sel = idx.numel()
    if keep_last is not None:
        idx = idx[-keep_last:]
    prev = torch.cat([obs0[None], obs[:-1]], 0).reshape(K * B, -1)[idx].double()
    nxt = torch.where(done[..., None], traj["term_obs"][:K], obs).reshape(K * B, -1)[idx].double()
    u = traj["u"][:K].reshape(K * B, -1)[idx].double()
    t = e.reshape(-1)[idx].double() * dt

    def state(o):
        if env.dynamics_mode == "Unicycle":
            return torch.stack([o[:, 0], o[:, 1], torch.atan2(o[:, 3], o[:, 2])], 1)
        s = o.clone()
        s[:, ::2] *= 100.0
        s[:, 1::2] *= 30.0
        return s

    x, xn = state(prev), state(nxt)
    if env.dynamics_mode == "Unicycle":
        F = torch.stack([torch.cos(x[:, 2]) * u[:, 0], torch.sin(x[:, 2]) * u[:, 0], u[:, 1]], 1) + 0.0
    else:
        pos, vel = x[:, ::2], x[:, 1::2]
        vdes = torch.full_like(vel, 30.0)
        vdes[:, 0] -= 10 * torch.sin(0.2 * t)
        acc = 4.0 * (vdes - vel)
        d01, d12, d24 = pos[:, 0] - pos[:, 1], pos[:, 1] - pos[:, 2], pos[:, 2] - pos[:, 4]
        acc[:, 1] -= 20.0 * d01 * (d01 < 6.0)
        acc[:, 2] -= 20.0 * d12 * (d12 < 6.0)
        acc[:, 3] = 0.0
        acc[:, 4] -= 20.0 * d24 * (d24 < 13.0)
        F = torch.zeros_like(x)
        F[:, ::2] = vel
        F[:, 1::2] = acc
        F[:, 7] += 50.0 * u[:, 0]
    # a true division, as numpy's and the kernel's: by a host scalar torch multiplies by the reciprocal instead
    return x, ((xn - x) - dt * F) / torch.tensor(dt, dtype=torch.float64, device=x.device), n_sel


def host_loop(dm, env, traj, obs0, step0, K, every):
    """(b): main.py:110-113 on the host, from the device arrays."""
    import numpy as np
    obs, u = traj["obs"][:K].cpu().numpy(), traj["u"][:K].cpu().numpy()
    term, done = traj["term_obs"][:K].cpu().numpy(), traj["done"][:K].cpu().numpy() != 0
    prev, c = obs0.cpu().numpy(), step0.cpu().numpy().astype(np.int64)
    for j in range(K):
        e = c + 1
        nxt = np.where(done[j][:, None], term[j], obs[j])
        sel = e % every == 0
        if sel.any():
            dm.append_transition(dm.get_state(prev[sel]), u[j][sel], dm.get_state(nxt[sel]), t_batch=e[sel] * env.dt)
        c = np.where(done[j], 0, e)
        prev = obs[j]


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
    return ts[len(ts) // 2]


def measure(name, B, K, keep_last, a):
    import torch

    from rcbf_amd import _lib
    from rcbf_amd.dynamics import DynamicsModel
    dev = torch.device("cuda", 0)
    env = Env(name, B)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    traj, obs0, step0 = make_trajectory(env, K, gen)
    dm = DynamicsModel(types.SimpleNamespace(dynamics_mode=env.dynamics_mode, dt=env.dt),
                       types.SimpleNamespace(cuda=True, gp_model_size=2000))
    dm.fit_gp_model = lambda *x, **k: None
    every = 2
    # the two device paths agree on these inputs
    xs, ds, n_sel = dm.trajectory_rows(env, traj, obs0, step0, every=every, keep_last=keep_last)
    xt, dt_, n_t = torch_rows(env, traj, obs0, step0, K, every, keep_last)
    assert n_sel == n_t and xs.shape == xt.shape, (n_sel, n_t, xs.shape, xt.shape)
    rows = xs.shape[0]
    out = {"env": name, "B": B, "K": K, "every": every, "keep_last": keep_last, "n_selected": n_sel, "rows": rows,
           "max_abs_x_vs_torch": float((xs - xt).abs().max()), "max_abs_d_vs_torch": float((ds - dt_).abs().max())}
    print(json.dumps(out), flush=True)
    # both are device fp64 with the same library sin / cos / atan2 and the same operation order: equal states, and
    # d within the GPU tests' bound for a column a transcendental reaches
    assert out["max_abs_x_vs_torch"] == 0.0 and out["max_abs_d_vs_torch"] <= 1e-12, "the two device paths disagree"
    # the launches alone, into preallocated arrays
    lib = _lib.load()
    n_alloc = max(rows, 1)
    so = torch.empty(2, n_alloc, env.n_s, dtype=torch.float64, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    scr = torch.empty(lib.rcbf_traj_pack_gp_scratch_bytes(B, K) // 8, dtype=torch.int64, device=dev)
    pitch = traj["obs"].stride(0) // env.n_o

    def launch():
        rc = lib.rcbf_traj_pack_gp_f64(_lib.ptr(so[0]), _lib.ptr(so[1]), _lib.ptr(cnt), _lib.ptr(scr), B, K, pitch,
                                       env.n_o, env.n_u, _lib.ptr(obs0), _lib.ptr(step0), _lib.ptr(traj["obs"]),
                                       _lib.ptr(traj["term_obs"]), _lib.ptr(traj["u"]), _lib.ptr(traj["done"]), env.dt,
                                       1, every, n_alloc, _lib.stream_of(dev))
        assert rc == 0

    r_us, t_us = [], []
    for _ in range(a.rounds):  # alternating pairs
        r_us.append(timed(lambda: dm.trajectory_rows(env, traj, obs0, step0, every=every, keep_last=keep_last),
                          a.reps))
        t_us.append(timed(lambda: torch_rows(env, traj, obs0, step0, K, every, keep_last), a.reps))
    l_us = timed(launch, a.reps)
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_loop(dm, env, traj, obs0, step0, K, every)
        host.append((time.perf_counter() - t0) * 1e6)
    nbytes = K * B * (4 * (env.n_o + env.n_u) + 1) + rows * 16 * env.n_s
    out.update({"rows_us_rounds": [round(v, 1) for v in r_us], "torch_us_rounds": [round(v, 1) for v in t_us],
                "rows_faster_in_every_pair": all(r < t for r, t in zip(r_us, t_us)),
                "torch_over_rows_median": round(sorted(t_us)[len(t_us) // 2] / sorted(r_us)[len(r_us) // 2], 2),
                "launch_us": round(l_us, 1), "algorithmic_bytes": nbytes,
                "launch_TB_per_s": round(nbytes / l_us / 1e6, 3) if keep_last is None else None,
                "host_loop_us": [round(v) for v in host]})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="cars,unicycle")
    ap.add_argument("--shapes", default="65536x20,64x1000")
    ap.add_argument("--keep-last", default="none,3000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "exp_traj_gp.py measures on the GPU"
    for name in a.envs.split(","):
        for shape in a.shapes.split(","):
            B, K = (int(v) for v in shape.split("x"))
            for kl in a.keep_last.split(","):
                measure(name, B, K, None if kl == "none" else int(kl), a)


if __name__ == "__main__":
    main()
