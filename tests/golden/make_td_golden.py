#!/usr/bin/env python
"""Generate tests/golden/td_target.npz: the reference's own SAC target block
(rcbf_sac/sac_cbf.py:130-136) on fixed inputs.

CONTAINER-ONLY, like make_golden.py (whose import stubs and exact-QP patch it
uses) and make_policy_golden.py (whose observations it uses): it imports the
read-only reference, runs on the CPU, and only the .npz it writes is
committed.  For cars (n_o 10, n_u 1) and unicycle with 3 hazards (7, 2), at
hidden size 64, 130 rows (65 observations of the reference env, and the same
65 scaled x20, every other one x-20), the layer of make_sac_update
(gamma_b = 20, k_d = 1.5, l_p = 0.03, prior disturbance):

  <env>_psd_<name>, _csd_<name>   GaussianPolicy / QNetwork state dicts, biases redrawn U(-0.1, 0.1), the log-std
                                  head's weights x4 (make_policy_golden.py says why)
  <env>_action_scale/_action_bias
  <env>_obs, _eps                 eps: torch's draws for rsample (re-seeded, _standard_normal on rsample's shape;
                                  asserted to reproduce sample's action)
  <env>_action, _log_prob, _mean  GaussianPolicy.sample(obs)
  <env>_safe                      RCBF_SAC.get_safe_action(obs, action, dynamics_model)
  <env>_q1, _q2                   critic_target(obs, safe)
  <env>_reward, _mask, _next_q    next_q_value for alpha = 0.2, gamma = 0.99
  unicycle_hazards

Asserted per env: some rows saturate the tanh, some reach each log-std clamp,
q1 < q2 and q2 < q1 both occur, and the QP's active set of every row is the
same in the reference and in the fp64 oracle chain (port sample -> oracle safe
action), for which the seed is searched: no row needs leaving out of the
end-to-end comparison.
"""
import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden as MG  # noqa: E402
import make_policy_golden as MPG  # noqa: E402

HIDDEN, ALPHA, GAMMA, GAMMA_B = 64, 0.2, 0.99, 20.0
MODES = {"cars": "SimulatedCars", "unicycle": "Unicycle"}


class _A:
    gp_model_size = 2000
    cuda = False


class _Agent:  # the attribute RCBF_SAC.get_safe_action touches
    pass


def one(name, Env, seed, diff_cbf_qp, dynamics):
    """The fixture of one env for one seed, or the reason the seed does not serve."""
    import _critic_port as CP
    from oracle import oracle as O
    from rcbf_sac import sac_cbf
    from rcbf_sac.model import GaussianPolicy, QNetwork
    from torch.distributions.utils import _standard_normal
    np.random.seed(seed)
    rng = np.random.default_rng(seed)
    env = Env()
    hazards = None
    if name == "unicycle":
        env.hazards_locations = env.hazards_locations[:3]
        hazards = env.hazards_locations.astype(np.float64)
    n_o, n_u = env.observation_space.shape[0], env.action_space.shape[0]
    torch.manual_seed(seed)
    pol = GaussianPolicy(n_o, n_u, HIDDEN, env.action_space)
    crit = QNetwork(n_o, n_u, HIDDEN)
    with torch.no_grad():
        for m in (pol.linear1, pol.linear2, pol.mean_linear, pol.log_std_linear,
                  *(getattr(crit, f"linear{k}") for k in range(1, 7))):
            m.bias.uniform_(-0.1, 0.1)
        pol.log_std_linear.weight.mul_(4.0)
    real = MPG.observations(env, rng, 65)
    sign = np.where(np.arange(65) % 2, -20.0, 20.0)[:, None]
    obs = np.concatenate([real, (sign * real).astype(np.float32)])
    B = obs.shape[0]
    reward = rng.normal(0.0, 1.0, (B, 1)).astype(np.float32)
    mask = rng.integers(0, 2, (B, 1)).astype(np.float32)
    agent = _Agent()
    agent.cbf_layer = MG._patch_layer(diff_cbf_qp.CBFQPLayer(env, _A(), gamma_b=GAMMA_B, k_d=1.5, l_p=0.03))
    dm = dynamics.DynamicsModel(env, _A())
    obs_t = torch.tensor(obs)
    with torch.no_grad():
        mean, log_std = pol.forward(obs_t)
        raw = pol.log_std_linear(torch.relu(pol.linear2(torch.relu(pol.linear1(obs_t)))))
        torch.manual_seed(seed + 1000)
        eps = _standard_normal(mean.shape, dtype=mean.dtype, device=mean.device)  # Normal.rsample's draw
        torch.manual_seed(seed + 1000)
        action, log_prob, mean_action = pol.sample(obs_t)
        x_t = mean + eps * log_std.exp()
        assert torch.equal(action, torch.tanh(x_t) * pol.action_scale + pol.action_bias), "eps is not rsample's draw"
        try:
            safe = sac_cbf.RCBF_SAC.get_safe_action(agent, obs_t, action, dm)
        except Exception as e:  # the patched exact QP found no KKT point on some row
            return None, f"reference QP: {e}"
        q1, q2 = crit(obs_t, safe)
        next_q = torch.tensor(reward) + torch.tensor(mask) * GAMMA * (torch.min(q1, q2) - ALPHA * log_prob)
    if not ((raw > 2).any() and (raw < -20).any()):
        return None, "log-std clamps not both reached"
    if not ((x_t.abs() > 9.5).any() and (x_t.abs() < 1).any()):
        return None, "no saturated / no open tanh"
    if not ((q1 < q2).any() and (q2 < q1).any()):
        return None, "min(q1, q2) takes one side only"
    # the fp64 oracle chain's active sets against the reference's
    psd = {k: v.numpy() for k, v in pol.state_dict().items()}
    scale, bias = pol.action_scale.numpy(), pol.action_bias.numpy()
    a64 = CP.sample(psd, scale, bias, obs, eps.numpy())[0]
    mode = MODES[name]
    mu, sg = O.predict_disturbance_prior(mode, B)
    _, aux = O.safe_action_diff(mode, O.get_state_f32(mode, obs), a64.astype(np.float32), mu.astype(np.float32),
                                sg.astype(np.float32), GAMMA_B, hazards=hazards)
    if (aux["status"] != 0).any():
        return None, "oracle QP status"
    m, n = aux["Gn"].shape[1:]
    subsets = [S for k in range(0, n + 1) for S in itertools.combinations(range(m), k)]
    ref_active = np.zeros((B, m), bool)
    for b, si in enumerate(agent.cbf_layer._last_active.tolist()):
        ref_active[b, list(subsets[si])] = True
    if not np.array_equal(ref_active, aux["active"]):
        return None, f"active sets differ on rows {np.flatnonzero((ref_active != aux['active']).any(axis=1)).tolist()}"
    out = {f"{name}_psd_{k}": v.astype(np.float32) for k, v in psd.items()}
    out.update({f"{name}_csd_{k}": v.numpy().astype(np.float32) for k, v in crit.state_dict().items()})
    out.update({f"{name}_action_scale": scale.astype(np.float32), f"{name}_action_bias": bias.astype(np.float32),
                f"{name}_obs": obs, f"{name}_eps": eps.numpy(), f"{name}_action": action.numpy(),
                f"{name}_log_prob": log_prob.numpy(), f"{name}_mean": mean_action.numpy(), f"{name}_safe": safe.numpy(),
                f"{name}_q1": q1.numpy(), f"{name}_q2": q2.numpy(), f"{name}_reward": reward, f"{name}_mask": mask,
                f"{name}_next_q": next_q.numpy()})
    if hazards is not None:
        out["unicycle_hazards"] = hazards
    return out, "ok"


def main():
    SimulatedCarsEnv, UnicycleEnv, diff_cbf_qp, _, dynamics = MG._import_reference()
    out = {"alpha": np.float64(ALPHA), "gamma": np.float64(GAMMA), "gamma_b": np.float64(GAMMA_B)}
    for name, Env in (("cars", SimulatedCarsEnv), ("unicycle", UnicycleEnv)):
        for seed in range(1, 200):
            got, why = one(name, Env, seed, diff_cbf_qp, dynamics)
            print(name, "seed", seed, why)
            if got is not None:
                out.update(got)
                out[f"{name}_seed"] = np.int64(seed)
                break
        else:
            raise SystemExit(f"no seed serves {name}")
    path = os.path.join(HERE, "td_target.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
