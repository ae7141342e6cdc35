"""Policy forward: rcbf_policy_act (one launch, DevicePolicy.act) against the
same weights as a torch module's sample() on the same device, H = 256, cars
(n_o 10, n_u 1) and unicycle (7, 2) shapes, B = 1, 256, 4 096, 65 536.

Both sides sample (ours with the in-kernel draws, torch with its generator) and
are hipGraph-timed: 20 calls per graph, HIP events around a replay, best of 3
replays, the two sides alternating, the whole measurement repeated `--repeats`
times (the spread is reported).  B = 1 is also timed eagerly from the host call
to the result on the host (median of 200 calls, each ending in the 4- or 8-byte
read of the action).  `tflops` = 2 (n_o H + H^2 + heads H) B / time, heads =
2 n_u; a whole-call rate, not a kernel's share of peak.
Usage: python scripts/policy_bench.py [--out FILE] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sac-rcbf_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from rcbf_amd.policy import DevicePolicy  # noqa: E402

H = 256
SHAPES = {"cars": (10, 1), "unicycle": (7, 2)}


class TorchPolicy(nn.Module):
    """A tanh-Gaussian SAC actor with the reference policy's layer names and
    sample() outputs (action, log-probability, deterministic action)."""

    def __init__(self, n_o, n_u, hidden):
        super().__init__()
        self.linear1, self.linear2 = nn.Linear(n_o, hidden), nn.Linear(hidden, hidden)
        self.mean_linear, self.log_std_linear = nn.Linear(hidden, n_u), nn.Linear(hidden, n_u)
        self.register_buffer("action_scale", torch.ones(n_u))
        self.register_buffer("action_bias", torch.zeros(n_u))

    def forward(self, obs):
        h = torch.relu(self.linear2(torch.relu(self.linear1(obs))))
        return self.mean_linear(h), self.log_std_linear(h).clamp(-20, 2)

    def sample(self, obs):
        mean, log_std = self.forward(obs)
        dist = torch.distributions.Normal(mean, log_std.exp(), validate_args=False)  # no host read: capturable
        x = dist.rsample()
        y = torch.tanh(x)
        logp = (dist.log_prob(x) - torch.log(self.action_scale * (1 - y * y) + 1e-6)).sum(1, keepdim=True)
        return y * self.action_scale + self.action_bias, logp, torch.tanh(mean) * self.action_scale + self.action_bias


def graph_of(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def eager_us(fn, n=200):
    for _ in range(20):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_bench needs the MI355X: no timing is taken without it")
    dev = torch.device("cuda", 0)
    rows = []
    for name, (n_o, n_u) in SHAPES.items():
        torch.manual_seed(0)
        module = TorchPolicy(n_o, n_u, H).to(dev)
        pol = DevicePolicy(module, seed=1)
        flops_row = 2 * (n_o * H + H * H + 2 * n_u * H)
        for B in (1, 256, 4096, 65536):
            obs = torch.rand(B, n_o, device=dev)
            out = torch.empty(B, n_u, device=dev)
            with torch.no_grad():
                # results must agree before a time means anything: the deterministic action of both sides
                ref = module.sample(obs)[2]
                err = float((pol.act(obs, evaluate=True) - ref).abs().max())
                assert err < 1e-5, err
                g_ours = graph_of(lambda: pol.act(obs, out=out, counter=0), args.reps)
                g_torch = graph_of(lambda: module.sample(obs), args.reps)
                ours, theirs = [], []
                for _ in range(args.repeats):
                    a, b = [], []
                    for _ in range(3):  # alternating
                        a.append(replay_us(g_ours, args.reps))
                        b.append(replay_us(g_torch, args.reps))
                    ours.append(min(a))
                    theirs.append(min(b))
                row = {"env": name, "B": B, "H": H, "graph_us_ours": round(min(ours), 2),
                       "graph_us_ours_spread": [round(min(ours), 2), round(max(ours), 2)],
                       "graph_us_torch": round(min(theirs), 2),
                       "graph_us_torch_spread": [round(min(theirs), 2), round(max(theirs), 2)],
                       "speedup": round(min(theirs) / min(ours), 2),
                       "tflops_ours": round(flops_row * B / min(ours) / 1e6, 3),
                       "tflops_torch": round(flops_row * B / min(theirs) / 1e6, 3), "max_abs_diff_mean_action": err}
                if B == 1:
                    row["eager_us_ours"] = round(eager_us(lambda: pol.act(obs, out=out).cpu()), 1)
                    row["eager_us_torch"] = round(eager_us(lambda: module.sample(obs)[0].cpu()), 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del g_ours, g_torch
    res = {"what": "policy forward, rcbf_policy_act vs torch module.sample(), hipGraph of %d calls" % args.reps,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
