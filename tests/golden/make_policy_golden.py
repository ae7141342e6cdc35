#!/usr/bin/env python
"""Generate tests/golden/policy.npz from the reference's own GaussianPolicy.

CONTAINER-ONLY, like make_golden.py (whose import stubs it uses): it imports
the read-only reference, runs on the CPU, and only the .npz it writes is
committed.  For cars (n_o 10, n_u 1) and unicycle (7, 2) at hidden size 64:

  <env>_sd_<name>        the seeded module's state_dict (fp32)
  <env>_action_scale/_action_bias   from the env's action space (model.py:76-84)
  <env>_obs              (130, n_o) f32: 65 observations of the reference env
                         (a reset, then steps under uniform random actions),
                         and the same 65 scaled x20, every other one x-20, so
                         that some tanh saturate and some log_std reach both
                         clamps (asserted below)
  <env>_mean, _log_std   GaussianPolicy.forward(obs)   (model.py:86-92)
  <env>_action_mean      GaussianPolicy.sample(obs)[2] (model.py:105)

The default init has zero biases (model.py:11-14); they are redrawn U(-0.1, 0.1)
from the same seeded generator so that a dropped bias cannot pass, and the
log-std head's weights are scaled x4: at its initial scale the x20 rows reach
neither clamp on cars (raw log_std within [-15, 3] over 60 seeds), and a
trained head is not at its initial scale.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

HIDDEN = 64
SEEDS = {"cars": 4, "unicycle": 53}


def observations(env, rng, n):
    obs = [np.asarray(env.reset(), np.float32)]
    while len(obs) < n:
        o, _, done, _ = env.step(rng.uniform(-1.0, 1.0, env.action_space.shape))
        obs.append(np.asarray(o, np.float32))
        if done:
            obs.append(np.asarray(env.reset(), np.float32))
    return np.stack(obs[:n])


def main():
    SimulatedCarsEnv, UnicycleEnv, *_ = MG._import_reference()
    from rcbf_sac.model import GaussianPolicy
    out = {}
    for name, Env in (("cars", SimulatedCarsEnv), ("unicycle", UnicycleEnv)):
        np.random.seed(SEEDS[name])
        rng = np.random.default_rng(SEEDS[name])
        env = Env()
        n_o, n_u = env.observation_space.shape[0], env.action_space.shape[0]
        torch.manual_seed(SEEDS[name])
        pol = GaussianPolicy(n_o, n_u, HIDDEN, env.action_space)
        with torch.no_grad():
            for m in (pol.linear1, pol.linear2, pol.mean_linear, pol.log_std_linear):
                m.bias.uniform_(-0.1, 0.1)
            pol.log_std_linear.weight.mul_(4.0)
        real = observations(env, rng, 65)
        sign = np.where(np.arange(65) % 2, -20.0, 20.0)[:, None]
        obs = np.concatenate([real, (sign * real).astype(np.float32)])
        with torch.no_grad():
            mean, log_std = pol.forward(torch.tensor(obs))
            raw = pol.log_std_linear(torch.relu(pol.linear2(torch.relu(pol.linear1(torch.tensor(obs))))))
            act_mean = pol.sample(torch.tensor(obs))[2]
        assert (raw > 2).any() and (raw < -20).any(), (name, float(raw.min()), float(raw.max()))
        assert (mean.abs() > 9).any() and (mean.abs() < 1).any(), name  # tanh saturated in fp32 / far from it
        for k, v in pol.state_dict().items():
            out[f"{name}_sd_{k}"] = v.numpy().astype(np.float32)
        out[f"{name}_action_scale"] = pol.action_scale.numpy().astype(np.float32)
        out[f"{name}_action_bias"] = pol.action_bias.numpy().astype(np.float32)
        out[f"{name}_obs"] = obs
        out[f"{name}_mean"] = mean.numpy()
        out[f"{name}_log_std"] = log_std.numpy()
        out[f"{name}_action_mean"] = act_mean.numpy()
    path = os.path.join(HERE, "policy.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
