"""The twin critic's inference forward on the device, one launch per call.

The first half of RCBF_SAC.update_parameters (rcbf_sac/sac_cbf.py:130-136)
evaluates critic_target under no_grad: six Linear launches, the concatenation
and the elementwise target in torch.  DeviceCritic packs a QNetwork
(rcbf_sac/model.py:34-61: linear1..3 and linear4..6) once into the layout
rcbf_critic_q reads (include/rcbf_hip.h) and computes

    q(obs, act)            q1, q2 = QNetwork.forward(obs, act)
    td_target(...)         reward + mask * gamma * (min(q1, q2) - alpha * log_pi)

in one kernel each (csrc/rcbf_critic.hip), fp32, every sum one fmaf chain in a
fixed order: a row's values do not depend on the batch around it.  Inference
only -- the critic's loss and its backward stay in torch on the module;
refresh() re-packs it after an optimiser step or a soft_update.
"""
import torch

from . import _lib
from .policy import _a_operand


def packed_floats(n_o, n_u, hidden):
    """rcbf_critic_packed_floats as a formula (include/rcbf_hip.h)."""
    k1 = (n_o + n_u + 1) & ~1
    return 2 * (hidden * (k1 + hidden + 3) + 4)


class DeviceCritic:
    """module: anything with linear1 .. linear6 as the reference's QNetwork
    has them (linear1-3 the first net, linear4-6 the second)."""

    def __init__(self, module, device=None):
        for k in range(1, 7):
            if not hasattr(getattr(module, f"linear{k}", None), "weight"):
                raise ValueError(f"critic module has no linear{k}")
        self.module = module
        w1 = module.linear1.weight
        # n_in = n_o + n_u: the layout depends on the sum alone; a call's action width says where obs ends
        self.hidden, self.n_in = int(w1.shape[0]), int(w1.shape[1])
        H, n_in = self.hidden, self.n_in
        if not (2 <= n_in <= 18):
            raise ValueError(f"the critic kernel takes 2 .. 18 inputs (1 .. 16 observation components and 1 or 2 "
                             f"actions), got {n_in}")
        if H % 32 or not (32 <= H <= 256):
            raise ValueError(f"hidden size must be a multiple of 32 in [32, 256], got {H}")
        for a, b, c in ((module.linear1, module.linear2, module.linear3), (module.linear4, module.linear5, module.linear6)):
            if tuple(a.weight.shape) != (H, n_in) or tuple(b.weight.shape) != (H, H) or tuple(c.weight.shape) != (1, H):
                raise ValueError("critic module: layer shapes do not chain")
        self.device = torch.device(device) if device is not None else w1.device
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.packed = torch.zeros(packed_floats(n_in - 1, 1, H), dtype=torch.float32, device=self.device)
        self.refresh()

    def refresh(self):
        """Re-pack the module's current weights into the same device buffer
        (after an optimiser step or soft_update): no reallocation, so a
        captured graph that holds the buffer's address stays valid.  Torch
        ops, set-up only."""
        m, H, n_in, dev = self.module, self.hidden, self.n_in, self.device
        k1 = (n_in + 1) & ~1

        def f32(t):
            return t.detach().to(device=dev, dtype=torch.float32)

        with torch.no_grad():
            off = 0
            for l1, l2, l3 in ((m.linear1, m.linear2, m.linear3), (m.linear4, m.linear5, m.linear6)):
                w1 = torch.zeros(H, k1, dtype=torch.float32, device=dev)
                w1[:, :n_in] = f32(l1.weight)
                for t, size in ((_a_operand(w1, 1), H * k1), (f32(l1.bias), H), (_a_operand(f32(l2.weight), 4), H * H),
                                (f32(l2.bias), H), (f32(l3.weight).reshape(-1), H), (f32(l3.bias), 4)):
                    self.packed[off:off + t.numel()].copy_(t)
                    off += size
            assert off == self.packed.numel()
        return self

    def _check(self, t, name, width):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == width):
            raise ValueError(f"{name} must be a float32 tensor of shape (B, {width})")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the critic on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    def _check_inputs(self, obs, act):
        """-> (B, n_o, n_u): the action's width splits the input [obs | act]."""
        n_u = int(act.shape[1]) if torch.is_tensor(act) and act.dim() == 2 else 0
        if n_u not in (1, 2) or not (1 <= self.n_in - n_u <= 16):
            raise ValueError(f"act must be a float32 tensor of shape (B, 1) or (B, 2) beside obs (B, {self.n_in} - n_u)")
        self._check(obs, "obs", self.n_in - n_u)
        self._check(act, "act", n_u)
        B = int(obs.shape[0])
        if act.shape[0] != B:
            raise ValueError(f"act has {act.shape[0]} rows, obs {B}")
        return B, self.n_in - n_u, n_u

    def _column(self, t, name, B):
        """A (B, 1) or (B,) fp32 column, as the reference's unsqueezed reward / mask batches."""
        if torch.is_tensor(t) and t.dim() == 1:
            t = t.unsqueeze(1)
        self._check(t, name, 1)
        if t.shape[0] != B:
            raise ValueError(f"{name} has {t.shape[0]} rows, obs {B}")
        return t

    def q(self, obs, act, out=None):
        """obs (B, n_o), act (B, n_u) f32 on the critic's device -> (q1, q2),
        each (B, 1) f32 (into the pair `out` when given).  One library call."""
        B, n_o, n_u = self._check_inputs(obs, act)
        if out is None:
            out = (torch.empty(B, 1, dtype=torch.float32, device=self.device),
                   torch.empty(B, 1, dtype=torch.float32, device=self.device))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError("out must be (q1, q2)")
            out = tuple(self._column(t, f"out[{k}]", B) for k, t in enumerate(out))
        if self.device.type != "cuda":
            raise ValueError("DeviceCritic.q needs HIP device tensors")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rcbf_critic_q(_lib.ptr(self.packed), n_o, n_u, self.hidden, B, _lib.ptr(obs),
                                   _lib.ptr(act), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_critic_q")
        return out

    def td_target(self, obs, act, reward, mask, log_pi, alpha, gamma, out=None, q_out=None):
        """reward + mask * gamma * (min(q1, q2) - alpha * log_pi) with
        (q1, q2) = q(obs, act), (B, 1) f32, one launch (sac_cbf.py:134-136).
        reward, mask and log_pi are (B, 1) or (B,) f32; alpha is a float or a
        one-element f32 tensor on the critic's device, which the kernel reads
        itself (automatic entropy tuning: no host read); `q_out`, a pair of
        (B, 1) tensors, also receives the Q-values."""
        B, n_o, n_u = self._check_inputs(obs, act)
        reward, mask, log_pi = (self._column(t, n, B) for t, n in ((reward, "reward"), (mask, "mask"), (log_pi, "log_pi")))
        alpha_dev = None
        if torch.is_tensor(alpha):
            if alpha.numel() != 1 or alpha.dtype != torch.float32 or alpha.device != self.device:
                raise ValueError(f"alpha as a tensor must be one float32 element on {self.device}")
            alpha_dev, alpha = alpha.detach(), 0.0
        if out is None:
            out = torch.empty(B, 1, dtype=torch.float32, device=self.device)
        else:
            out = self._column(out, "out", B)
        if q_out is not None:
            if not isinstance(q_out, (tuple, list)) or len(q_out) != 2:
                raise ValueError("q_out must be (q1, q2)")
            q_out = tuple(self._column(t, f"q_out[{k}]", B) for k, t in enumerate(q_out))
        if self.device.type != "cuda":
            raise ValueError("DeviceCritic.td_target needs HIP device tensors")
        lib = _lib.load()
        with torch.cuda.device(self.device):
            rc = lib.rcbf_critic_td_target(_lib.ptr(self.packed), n_o, n_u, self.hidden, B, _lib.ptr(obs),
                                           _lib.ptr(act), _lib.ptr(reward), _lib.ptr(mask), _lib.ptr(log_pi),
                                           float(alpha), _lib.ptr(alpha_dev), float(gamma), _lib.ptr(out),
                                           _lib.ptr(q_out[0]) if q_out else None,
                                           _lib.ptr(q_out[1]) if q_out else None, _lib.stream_of(self.device))
        _lib.check(rc, "rcbf_critic_td_target")
        return out
