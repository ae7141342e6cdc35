#!/usr/bin/env python
"""Time the SAC target block (rcbf_sac/sac_cbf.py:130-136) on the device:
rcbf_amd.sac_cbf.td_target (three library calls) against a torch restatement
of the same block (reference-shaped nn.Modules, this repo's get_safe_action in
the middle), cars config, prior disturbance, host call to stream-complete.

    python scripts/td_target_timing.py [--batch 256] [--hidden 256] [--rounds 11] [--iters 200] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/td_target_timing.py --trace

The two variants alternate round by round in one process; a round is `iters`
calls between two synchronisations, and the figures are the median and the
range of the rounds' per-call times.  --trace runs only a short loop of each
library call at B = 256 and 4096 for a kernel trace (no timing printed); the
twin-Q kernel's share of the fp32-MFMA rate is its FLOPs, 2 nets x 2 (K1 H +
H H + H) per row, over the traced kernel time and 157.3 TFLOP/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sac-rcbf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_FP32_MFMA = 157.3e12


class Args:
    cuda = True


def modules(n_o, n_u, H):
    import torch.nn as nn

    class Policy(nn.Module):
        def __init__(self):
            super().__init__()
            self.linear1, self.linear2 = nn.Linear(n_o, H), nn.Linear(H, H)
            self.mean_linear, self.log_std_linear = nn.Linear(H, n_u), nn.Linear(H, n_u)
            self.action_scale, self.action_bias = torch.tensor(10.0), torch.tensor(0.0)

        def sample(self, state):  # model.py:86-106
            x = torch.relu(self.linear2(torch.relu(self.linear1(state))))
            mean = self.mean_linear(x)
            log_std = torch.clamp(self.log_std_linear(x), min=-20, max=2)
            normal = torch.distributions.Normal(mean, log_std.exp())
            x_t = normal.rsample()
            y_t = torch.tanh(x_t)
            action = y_t * self.action_scale + self.action_bias
            log_prob = normal.log_prob(x_t)
            log_prob -= torch.log(self.action_scale * (1 - y_t.pow(2)) + 1e-6)
            return action, log_prob.sum(1, keepdim=True), torch.tanh(mean) * self.action_scale + self.action_bias

    class Q(nn.Module):
        def __init__(self):
            super().__init__()
            for k, (i, o) in enumerate(((n_o + n_u, H), (H, H), (H, 1)) * 2, 1):
                setattr(self, f"linear{k}", nn.Linear(i, o))

        def forward(self, state, action):  # model.py:50-61
            xu = torch.cat([state, action], 1)
            x1 = self.linear3(torch.relu(self.linear2(torch.relu(self.linear1(xu)))))
            x2 = self.linear6(torch.relu(self.linear5(torch.relu(self.linear4(xu)))))
            return x1, x2

    torch.manual_seed(0)
    pol, q = Policy().to("cuda"), Q().to("cuda")
    pol.action_scale, pol.action_bias = pol.action_scale.to("cuda"), pol.action_bias.to("cuda")
    return pol, q


def setup(B, H):
    from rcbf_amd.critic import DeviceCritic
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.dynamics import DynamicsModel
    from rcbf_amd.envs import BatchedSimulatedCarsEnv
    from rcbf_amd.policy import DevicePolicy
    env = BatchedSimulatedCarsEnv(B, seed=1)
    env.reset()
    layer, dyn = CBFQPLayer(env, Args(), gamma_b=20.0), DynamicsModel(env, Args())
    pol, q = modules(env.n_o, env.n_u, H)
    g = torch.Generator(device="cuda").manual_seed(1)
    reward = torch.randn(B, 1, device="cuda", generator=g)
    mask = (torch.rand(B, 1, device="cuda", generator=g) > 0.1).float()
    return dict(layer=layer, dyn=dyn, pol=pol, q=q, dpol=DevicePolicy(pol), dq=DeviceCritic(q),
                obs=env.obs.clone().contiguous(), reward=reward, mask=mask, n_o=env.n_o, n_u=env.n_u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X: no timing without a device")
    from rcbf_amd.sac_cbf import get_safe_action, td_target
    alpha, gamma = 0.2, 0.99

    if a.trace:
        for B in (256, 4096):
            s = setup(B, a.hidden)
            act = torch.zeros(B, s["n_u"], device="cuda")
            for _ in range(50):
                td_target(s["dpol"], s["dq"], s["layer"], s["dyn"], s["obs"], s["reward"], s["mask"], alpha, gamma)
                s["dq"].q(s["obs"], act)
            torch.cuda.synchronize()
        return

    s = setup(a.batch, a.hidden)

    def fused():
        return td_target(s["dpol"], s["dq"], s["layer"], s["dyn"], s["obs"], s["reward"], s["mask"], alpha, gamma)

    def in_torch():
        with torch.no_grad():
            act, log_pi, _ = s["pol"].sample(s["obs"])
            act = get_safe_action(s["layer"], s["obs"], act, s["dyn"])
            q1, q2 = s["q"](s["obs"], act)
            return s["reward"] + s["mask"] * gamma * (torch.min(q1, q2) - alpha * log_pi)

    times = {"fused": [], "torch": []}
    for fn in (fused, in_torch):  # warm-up: code objects, GEMM selection
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in (("fused", fused), ("torch", in_torch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e6)
    k1 = (s["n_o"] + s["n_u"] + 1) // 2 * 2
    res = {"what": "sac target block, host call to stream-complete, us per call", "batch": a.batch, "hidden": a.hidden,
           "rounds": a.rounds, "iters": a.iters,
           "twin_q_flops_per_row": 2 * 2 * (k1 * a.hidden + a.hidden * a.hidden + a.hidden)}
    for name, t in times.items():
        res[name] = {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}
    res["speedup_median"] = res["torch"]["median_us"] / res["fused"]["median_us"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
