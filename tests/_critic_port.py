"""numpy fp64 port of the SAC target block (rcbf_sac/sac_cbf.py:130-136) on fp32
weights: GaussianPolicy.sample's log-probability (model.py:94-106, the actor
itself from tests/_policy_port.py), QNetwork.forward (model.py:50-61) and the
target formula -- the oracle of the critic kernels' tests.  Critic weights are
a dict with the module's state_dict names ("linear1.weight" .. "linear6.bias").

torch_* restate the same in torch CPU fp32 as the reference writes it; their
error against the port on the same inputs sets each check's allowance (bound):
8 x that error + 1e-7 x max |value|, nothing absolute beyond it."""
import numpy as np

import _policy_port as PP

EPS = 1e-6  # model.py:8
UNSATURATED = 4.0  # rows with max_c |pre_tanh| below it: 1 - y^2 >= 1.3e-3, far above fp32 rounding and EPS


def sample(psd, scale, bias, obs, z):
    """(action, log_pi (B,), mean_action, pre_tanh), fp64.  (x_t - mean)^2 / (2 var) is z^2 / 2."""
    mean, ls = PP.forward(psd, obs)
    z = np.asarray(z, np.float64)
    scale, bias = np.asarray(scale, np.float64), np.asarray(bias, np.float64)
    pre = mean + np.exp(ls) * z
    y = np.tanh(pre)
    lp = -0.5 * z * z - ls - 0.5 * np.log(2.0 * np.pi) - np.log(scale * (1.0 - y * y) + EPS)
    return y * scale + bias, lp.sum(axis=1), np.tanh(mean) * scale + bias, pre


def unsaturated(pre):
    return np.max(np.abs(pre), axis=1) < UNSATURATED


def q_forward(csd, obs, act):
    """(q1, q2), each (B,), fp64."""
    w = {k: np.asarray(v, np.float64) for k, v in csd.items()}
    xu = np.concatenate([np.asarray(obs, np.float64), np.asarray(act, np.float64)], axis=1)
    out = []
    for a, b, c in ((1, 2, 3), (4, 5, 6)):
        h = np.maximum(xu @ w[f"linear{a}.weight"].T + w[f"linear{a}.bias"], 0.0)
        h = np.maximum(h @ w[f"linear{b}.weight"].T + w[f"linear{b}.bias"], 0.0)
        out.append((h @ w[f"linear{c}.weight"].T + w[f"linear{c}.bias"])[:, 0])
    return out[0], out[1]


def target(reward, mask, gamma, q1, q2, alpha, log_pi):
    r, m, lp = (np.asarray(t, np.float64).reshape(-1) for t in (reward, mask, log_pi))
    return r + m * gamma * (np.minimum(q1, q2) - alpha * lp)


def seeded_critic(n_in, hidden, seed):
    """Xavier-uniform weights, non-zero biases, fp32, from a numpy seed."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, (o, i) in zip(range(1, 7), ((hidden, n_in), (hidden, hidden), (1, hidden)) * 2):
        a = np.sqrt(6.0 / (i + o))
        sd[f"linear{k}.weight"] = rng.uniform(-a, a, (o, i)).astype(np.float32)
        sd[f"linear{k}.bias"] = rng.uniform(-0.1, 0.1, o).astype(np.float32)
    return sd


def torch_critic(csd):
    """A torch module with the reference QNetwork's attribute names holding csd."""
    import torch
    import torch.nn as nn

    class Q(nn.Module):
        def __init__(self):
            super().__init__()
            for k in range(1, 7):
                o, i = csd[f"linear{k}.weight"].shape
                setattr(self, f"linear{k}", nn.Linear(i, o))

    m = Q()
    m.load_state_dict({k: torch.tensor(np.asarray(v, np.float32)) for k, v in csd.items()})
    return m


def torch_sample(psd, scale, bias, obs, z):
    """GaussianPolicy.sample as model.py:94-106 writes it (Normal.log_prob on x_t), torch CPU fp32, with eps = z."""
    import torch
    import torch.nn.functional as F
    from torch.distributions import Normal
    t = {k: torch.tensor(np.asarray(v, np.float32)) for k, v in psd.items()}
    sc, bi = torch.tensor(np.asarray(scale, np.float32)), torch.tensor(np.asarray(bias, np.float32))
    with torch.no_grad():
        x = F.relu(F.linear(torch.tensor(np.asarray(obs, np.float32)), t["linear1.weight"], t["linear1.bias"]))
        x = F.relu(F.linear(x, t["linear2.weight"], t["linear2.bias"]))
        mean = F.linear(x, t["mean_linear.weight"], t["mean_linear.bias"])
        log_std = torch.clamp(F.linear(x, t["log_std_linear.weight"], t["log_std_linear.bias"]), PP.LOG_SIG_MIN,
                              PP.LOG_SIG_MAX)
        std = log_std.exp()
        normal = Normal(mean, std)
        x_t = mean + std * torch.tensor(np.asarray(z, np.float32))  # rsample with these draws
        y_t = torch.tanh(x_t)
        action = y_t * sc + bi
        log_prob = normal.log_prob(x_t)
        log_prob -= torch.log(sc * (1 - y_t.pow(2)) + EPS)
        log_prob = log_prob.sum(1)
        mean_action = torch.tanh(mean) * sc + bi
    return action.numpy(), log_prob.numpy(), mean_action.numpy()


def torch_q(csd, obs, act):
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, np.float32)) for k, v in csd.items()}
    with torch.no_grad():
        xu = torch.cat([torch.tensor(np.asarray(obs, np.float32)), torch.tensor(np.asarray(act, np.float32))], 1)
        out = []
        for a, b, c in ((1, 2, 3), (4, 5, 6)):
            x = F.relu(F.linear(xu, t[f"linear{a}.weight"], t[f"linear{a}.bias"]))
            x = F.relu(F.linear(x, t[f"linear{b}.weight"], t[f"linear{b}.bias"]))
            out.append(F.linear(x, t[f"linear{c}.weight"], t[f"linear{c}.bias"])[:, 0].numpy())
    return out[0], out[1]


def torch_target(csd, obs, act, reward, mask, gamma, alpha, log_pi):
    """sac_cbf.py:134-136 in torch CPU fp32 on (B, 1) columns."""
    import torch
    q1, q2 = (torch.tensor(q)[:, None] for q in torch_q(csd, obs, act))
    r, m, lp = (torch.tensor(np.asarray(t, np.float32).reshape(-1, 1)) for t in (reward, mask, log_pi))
    min_q = torch.min(q1, q2) - alpha * lp
    return (r + m * gamma * min_q)[:, 0].numpy()


def bound(ref, want):
    """(e_ref, allowance): the fp32 reference's max abs error against the port's value, and 8 e_ref + 1e-7 max|want|."""
    want = np.asarray(want, np.float64)
    e_ref = float(np.max(np.abs(np.asarray(ref, np.float64) - want))) if want.size else 0.0
    return e_ref, 8.0 * e_ref + 1e-7 * (float(np.max(np.abs(want))) if want.size else 0.0)


def check(name, got, ref, want, rows=None):
    """Assert |got - want| within bound(ref, want) on `rows` (all by default); print the figures first."""
    got, ref, want = (np.asarray(t, np.float64) for t in (got, ref, want))
    if rows is not None:
        got, ref, want = got[rows], ref[rows], want[rows]
    e_ref, allow = bound(ref, want)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    print(f"{name}: rows {len(want)} e_ref {e_ref:.3e} kernel {err:.3e} allowance {allow:.3e}")
    assert np.all(np.isfinite(got)), name
    assert err <= allow, (name, err, e_ref, allow)
    return err, e_ref, allow


WIDE_STD = -5.0  # log_std above it: x_t - mean = std z keeps ~1e-5 relative precision in fp32 (|mean| ~ 1)


def row_sets(pre, ls):
    """The row sets of a log_pi check, tightest first.  The reference forms (x_t - mean)^2 / (2 var): where log_std
    is near its lower clamp, x_t == mean in fp32 and the reference loses the whole 0.5 z^2 (its e_ref is ~1 there),
    so the unsaturated rows are split once more, lest those rows dilute the tight check."""
    open_ = unsaturated(pre)
    return (("unsaturated rows, log_std >= -5", open_ & (np.min(ls, axis=1) >= WIDE_STD)),
            ("unsaturated rows", open_), ("all rows", np.ones(len(open_), bool)))


def check_log_pi(name, got, ref, want, pre, ls):
    """log_pi on each row set under the set's own allowance (pre, ls: the port's pre-tanh values and log_std)."""
    for what, rows in row_sets(pre, ls):
        if not rows.any() and what != "all rows":  # a case without such rows: said, not hidden
            print(f"{name} log_pi, {what}: no rows")
            continue
        check(f"{name} log_pi, {what}", got, ref, want, rows)
