"""numpy fp64 port of the actor's forward (rcbf_sac/model.py:86-106) on fp32
weights: the oracle of the policy kernel's tests.  Weights are a dict with the
module's state_dict names ("linear1.weight", ... "mean_linear.weight",
"log_std_linear.weight", biases alike); action_scale / action_bias (n_u,)."""
import numpy as np

from oracle import oracle as O

LOG_SIG_MIN, LOG_SIG_MAX = -20.0, 2.0
ENV_SHAPES = {"cars": (10, 1), "unicycle": (7, 2)}  # n_o, n_u


def forward(sd, obs):
    """(mean, log_std), fp64; log_std clamped (model.py:86-92)."""
    w = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    x = np.asarray(obs, np.float64)
    h = np.maximum(x @ w["linear1.weight"].T + w["linear1.bias"], 0.0)
    h = np.maximum(h @ w["linear2.weight"].T + w["linear2.bias"], 0.0)
    mean = h @ w["mean_linear.weight"].T + w["mean_linear.bias"]
    ls = h @ w["log_std_linear.weight"].T + w["log_std_linear.bias"]
    return mean, np.clip(ls, LOG_SIG_MIN, LOG_SIG_MAX)


def pre_tanh(sd, obs, z=None):
    """mean (z None: evaluate=True, model.py:105) or mean + exp(log_std) z (model.py:96-98)."""
    mean, ls = forward(sd, obs)
    return mean if z is None else mean + np.exp(ls) * np.asarray(z, np.float64)


def act(sd, scale, bias, obs, z=None):
    """The action: tanh(pre_tanh) * action_scale + action_bias, fp64."""
    return np.tanh(pre_tanh(sd, obs, z)) * np.asarray(scale, np.float64) + np.asarray(bias, np.float64)


def implied_z(sd, scale, bias, obs, u):
    """The draw a sampled action u implies: (atanh((u - bias) / scale) - mean) / exp(log_std)."""
    mean, ls = forward(sd, obs)
    y = (np.asarray(u, np.float64) - np.asarray(bias, np.float64)) / np.asarray(scale, np.float64)
    return (np.arctanh(y) - mean) / np.exp(ls)


def draws(seed, rows, counter, n_u):
    """The kernel's z == NULL draws: the model step's, as fp32."""
    return O.model_step_normal(seed, rows, counter, n_u).astype(np.float32)


def seeded_weights(n_o, n_u, hidden, seed, gain=1.0):
    """Xavier-uniform weights like weights_init_ (model.py:11-14) but with
    non-zero biases, fp32, from a numpy seed (nothing of torch's generator)."""
    rng = np.random.default_rng(seed)

    def lin(o, i):
        a = gain * np.sqrt(6.0 / (i + o))
        return rng.uniform(-a, a, (o, i)).astype(np.float32), rng.uniform(-0.1, 0.1, o).astype(np.float32)

    sd = {}
    for name, (o, i) in (("linear1", (hidden, n_o)), ("linear2", (hidden, hidden)), ("mean_linear", (n_u, hidden)),
                         ("log_std_linear", (n_u, hidden))):
        sd[name + ".weight"], sd[name + ".bias"] = lin(o, i)
    return sd


def torch_module(sd, scale, bias):
    """A torch module with the reference policy's attribute names holding sd."""
    import torch
    import torch.nn as nn

    class Policy(nn.Module):
        def __init__(self):
            super().__init__()
            H, n_o = sd["linear1.weight"].shape
            n_u = sd["mean_linear.weight"].shape[0]
            self.linear1, self.linear2 = nn.Linear(n_o, H), nn.Linear(H, H)
            self.mean_linear, self.log_std_linear = nn.Linear(H, n_u), nn.Linear(H, n_u)
            self.action_scale = torch.tensor(np.asarray(scale, np.float32))
            self.action_bias = torch.tensor(np.asarray(bias, np.float32))

    m = Policy()
    m.load_state_dict({k: torch.tensor(np.asarray(v, np.float32)) for k, v in sd.items()})
    return m


def torch_reference(sd, scale, bias, obs, z=None):
    """The reference arithmetic in torch CPU fp32 (F.linear / relu / clamp /
    exp / tanh, model.py:86-106), whose error against the port sets the
    kernel's bound."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float32)) for k, v in sd.items()}
    with torch.no_grad():
        x = F.relu(F.linear(torch.tensor(np.asarray(obs, np.float32)), t["linear1.weight"], t["linear1.bias"]))
        x = F.relu(F.linear(x, t["linear2.weight"], t["linear2.bias"]))
        pre = F.linear(x, t["mean_linear.weight"], t["mean_linear.bias"])
        if z is not None:
            ls = torch.clamp(F.linear(x, t["log_std_linear.weight"], t["log_std_linear.bias"]), LOG_SIG_MIN, LOG_SIG_MAX)
            pre = pre + ls.exp() * torch.tensor(np.asarray(z, np.float32))
        u = torch.tanh(pre) * torch.tensor(np.asarray(scale, np.float32)) + torch.tensor(np.asarray(bias, np.float32))
    return u.numpy()


def bound(sd, scale, bias, obs, z=None):
    """(e_ref, bound): the reference arithmetic's max abs error against the
    port on these inputs, and the kernel's allowance 8 e_ref + 1e-7 scale."""
    e_ref = float(np.max(np.abs(torch_reference(sd, scale, bias, obs, z).astype(np.float64)
                                - act(sd, scale, bias, obs, z))))
    return e_ref, 8.0 * e_ref + 1e-7 * float(np.max(np.abs(scale)))
