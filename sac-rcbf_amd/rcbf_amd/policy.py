"""The actor's inference forward on the device, one launch per call.

agent.select_action (rcbf_sac/sac_cbf.py:59-85) takes its action from
GaussianPolicy.sample (rcbf_sac/model.py:86-106): four Linear launches and
about ten elementwise ones per step in torch, whose rounding depends on the
GEMM kernel the batch size selects.  DevicePolicy packs the module's weights
once into the layout rcbf_policy_act reads (include/rcbf_hip.h) and computes

    evaluate=True    tanh(mean) * action_scale + action_bias
    evaluate=False   tanh(mean + exp(log_std) * z) * action_scale + action_bias

in one kernel (csrc/rcbf_policy.hip), fp32, every sum one fmaf chain in a fixed
order: row i of a batched call is bit for bit the action a single-env call on
that row computes.  sample() adds GaussianPolicy.sample's log-probability and
mean action (csrc/rcbf_critic.hip), what the SAC target needs.  Inference only
-- no autograd; training keeps the torch module, and refresh() re-packs it
after an optimiser step.
"""
import torch

from . import _lib

MAX_OBS = 16


def packed_floats(n_o, n_u, hidden):
    """rcbf_policy_packed_floats as a formula (include/rcbf_hip.h)."""
    k1 = n_o + (n_o & 1)
    return hidden * (k1 + hidden + 2 + 2 * n_u) + 16


def check_policy_shape(n_o, n_u, hidden):
    if not (1 <= n_o <= MAX_OBS):
        raise ValueError(f"the policy kernel takes 1 .. {MAX_OBS} observation components, got {n_o}")
    if n_u not in (1, 2):
        raise ValueError(f"the policy kernel takes 1 or 2 actions, got {n_u}")
    if hidden % 32 or not (32 <= hidden <= 256):
        raise ValueError(f"hidden size must be a multiple of 32 in [32, 256], got {hidden}")


def _a_operand(w, k_per_lane):
    """(H, K) weights, K even -> the MFMA A-operand order of rcbf_hip.h:
    [unit block][k-step group][lane = 32 (k parity) + unit][k-step in group]."""
    H, K = w.shape
    g = K // (2 * k_per_lane)
    return w.reshape(H // 32, 32, g, k_per_lane, 2).permute(0, 2, 4, 1, 3).reshape(-1)


class DevicePolicy:
    """module: anything with linear1, linear2, mean_linear (or mean), an
    optional log_std_linear, and action_scale / action_bias (the reference's
    GaussianPolicy and DeterministicPolicy, or a user's own).  `seed` keys the
    in-kernel draws of act(evaluate=False) without z; `env_offset` is the global
    index of row 0 (a shard draws what the whole batch would)."""

    def __init__(self, module, device=None, seed=0, env_offset=0):
        for name in ("linear1", "linear2"):
            if not hasattr(module, name):
                raise ValueError(f"policy module has no {name}")
        head = getattr(module, "mean_linear", None)
        if head is None:
            head = getattr(module, "mean", None)
        if head is None or not hasattr(head, "weight"):
            raise ValueError("policy module has neither mean_linear nor mean")
        self.module = module
        self._mean_head = head
        self._log_std_head = getattr(module, "log_std_linear", None)
        w1 = module.linear1.weight
        self.hidden, self.n_o = int(w1.shape[0]), int(w1.shape[1])
        self.n_u = int(head.weight.shape[0])
        check_policy_shape(self.n_o, self.n_u, self.hidden)
        H = self.hidden
        if tuple(module.linear2.weight.shape) != (H, H) or int(head.weight.shape[1]) != H or (
                self._log_std_head is not None and tuple(self._log_std_head.weight.shape) != (self.n_u, H)):
            raise ValueError("policy module: layer shapes do not chain")
        self.device = torch.device(device) if device is not None else w1.device
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.seed = int(seed)
        self.env_offset = int(env_offset)
        self._counter = 0
        self.packed = torch.zeros(packed_floats(self.n_o, self.n_u, H), dtype=torch.float32, device=self.device)
        self.refresh()

    @property
    def has_log_std(self):
        return self._log_std_head is not None

    def refresh(self):
        """Re-pack the module's current weights into the same device buffer
        (after an optimiser step): no reallocation, so a captured graph that
        holds the buffer's address stays valid.  Torch ops, set-up only."""
        m, H, n_o, n_u, dev = self.module, self.hidden, self.n_o, self.n_u, self.device
        k1 = n_o + (n_o & 1)

        def f32(t):
            return torch.as_tensor(t).detach().to(device=dev, dtype=torch.float32)

        def vec(t):  # a scalar or (n_u,) value as n_u floats
            return f32(t).reshape(-1).expand(n_u) if f32(t).numel() == 1 else f32(t).reshape(n_u)

        with torch.no_grad():
            w1 = torch.zeros(H, k1, dtype=torch.float32, device=dev)
            w1[:, :n_o] = f32(m.linear1.weight)
            ls = self._log_std_head
            parts = [(_a_operand(w1, 1), H * k1), (f32(m.linear1.bias), H),
                     (_a_operand(f32(m.linear2.weight), 4), H * H), (f32(m.linear2.bias), H),
                     (f32(self._mean_head.weight).reshape(-1), n_u * H), (f32(self._mean_head.bias), 4),
                     (None if ls is None else f32(ls.weight).reshape(-1), n_u * H),
                     (None if ls is None else f32(ls.bias), 4),
                     (vec(getattr(m, "action_scale", 1.0)), 4), (vec(getattr(m, "action_bias", 0.0)), 4)]
            off = 0
            for t, size in parts:
                if t is not None:
                    self.packed[off:off + t.numel()].copy_(t)
                off += size
            assert off == self.packed.numel()
        return self

    def _check(self, t, name, width):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width):
            raise ValueError(f"{name} must be a float32 tensor of shape (B, {width})")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the policy on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    def act(self, obs, evaluate=False, out=None, z=None, seed=None, counter=None):
        """obs (B, n_o) f32 on the policy's device -> (B, n_u) f32 actions
        (into `out` when given).  evaluate=True is select_action's evaluation
        branch (the tanh of the mean); otherwise the action is sampled with the
        draws z (B, n_u) f32, or, without z, with the in-kernel Philox draws of
        (seed, env_offset + row, counter) -- oracle.model_step_normal.  The
        default counter increments per call.  One library call; nothing is read
        from the device."""
        self._check(obs, "obs", self.n_o)
        B = int(obs.shape[0])
        if not evaluate and self._log_std_head is None:
            raise NotImplementedError("evaluate=False needs a log-std head: the reference's DeterministicPolicy.sample "
                                      "shares one noise vector across rows, which is not reproduced")
        if out is None:
            out = torch.empty(B, self.n_u, dtype=torch.float32, device=self.device)
        else:
            self._check(out, "out", self.n_u)
            if out.shape[0] != B:
                raise ValueError(f"out has {out.shape[0]} rows, obs {B}")
        if z is not None:
            if evaluate:
                raise ValueError("z is the sampling noise: not used with evaluate=True")
            self._check(z, "z", self.n_u)
            if z.shape[0] != B:
                raise ValueError(f"z has {z.shape[0]} rows, obs {B}")
        if self.device.type != "cuda":
            raise ValueError("DevicePolicy.act needs HIP device tensors")
        if counter is None and not evaluate and z is None:
            counter = self._counter
            self._counter += 1
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rcbf_policy_act(_lib.ptr(self.packed), self.n_o, self.n_u, self.hidden, B, _lib.ptr(obs),
                                     _lib.ptr(out), _lib.POLICY_MEAN if evaluate else _lib.POLICY_SAMPLE, _lib.ptr(z),
                                     (self.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF,
                                     int(counter or 0) & 0xFFFFFFFFFFFFFFFF, self.env_offset,
                                     _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_policy_act")
        return out

    def sample(self, obs, z=None, seed=None, counter=None, out=None):
        """GaussianPolicy.sample (model.py:94-106): obs (B, n_o) ->
        (action (B, n_u), log_pi (B, 1), mean_action (B, n_u)), in one launch
        (rcbf_policy_sample).  The action is bit for bit act(evaluate=False)'s
        for the same z or (seed, counter) -- the default counter is act's, one
        per call -- and the mean action act(evaluate=True)'s; log_pi is the
        sample's log-probability with the tanh correction (the formula and its
        rounding order: include/rcbf_hip.h).  `out`: a triple of tensors to
        write into.  One library call; nothing is read from the device."""
        self._check(obs, "obs", self.n_o)
        B = int(obs.shape[0])
        if self._log_std_head is None:
            raise NotImplementedError("sample needs a log-std head: the reference's DeterministicPolicy.sample "
                                      "shares one noise vector across rows, which is not reproduced")
        if out is None:
            out = (torch.empty(B, self.n_u, dtype=torch.float32, device=self.device),
                   torch.empty(B, 1, dtype=torch.float32, device=self.device),
                   torch.empty(B, self.n_u, dtype=torch.float32, device=self.device))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 3:
                raise ValueError("out must be (action, log_pi, mean_action)")
            for t, name, width in zip(out, ("out[0]", "out[1]", "out[2]"), (self.n_u, 1, self.n_u)):
                self._check(t, name, width)
                if t.shape[0] != B:
                    raise ValueError(f"{name} has {t.shape[0]} rows, obs {B}")
        if z is not None:
            self._check(z, "z", self.n_u)
            if z.shape[0] != B:
                raise ValueError(f"z has {z.shape[0]} rows, obs {B}")
        if self.device.type != "cuda":
            raise ValueError("DevicePolicy.sample needs HIP device tensors")
        if counter is None and z is None:
            counter = self._counter
            self._counter += 1
        action, log_pi, mean_action = out
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rcbf_policy_sample(_lib.ptr(self.packed), self.n_o, self.n_u, self.hidden, B, _lib.ptr(obs),
                                        _lib.ptr(action), _lib.ptr(log_pi), _lib.ptr(mean_action), _lib.ptr(z),
                                        (self.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF,
                                        int(counter or 0) & 0xFFFFFFFFFFFFFFFF, self.env_offset, 1,
                                        _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_policy_sample")
        return action, log_pi, mean_action
