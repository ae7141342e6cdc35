"""What the episode statistics of a trajectory (rcbf_traj_episode_stats_f64:
count, scan, pack; rcbf_amd.EpisodeStats) cost, against the two things a user
of a trajectory plan could do before.  One process; prints one JSON line per
shape and, with --out, appends them to a file.

Arms, on the same synthetic cars-like trajectory (random fp32 reward and cost,
done with p = 1/300, random lengths and carries; pitch = B):
  call    rcbf_traj_episode_stats_f64 alone into preallocated arrays of n_ep
          rows (no host read): the device time the algorithmic bytes are
          divided by
  count   the count-only call (max_rows = 0, null carries): count + scan alone
  update  EpisodeStats.update(traj): the count-only call, the 8-byte read of
          n_ep, the allocation and the call that writes the records
  torch   the same statistics with torch ops on the device: an fp64 cumsum
          along the steps, the previous episode end of every step by a cummax,
          nonzero for the step-major compaction and gathers.  Its sums are
          differences of prefix sums, not the loop's additions: close, not
          bit-equal (the largest relative difference is printed)
  d2h     the device -> host copy of the three (K, B) arrays into pinned
          memory, which precedes any host loop over them
call / count / update / torch: device time between two events, warmed, the
median of --reps.  d2h: wall clock around the copies and a synchronise.
Algorithmic bytes: 9 per transition read by the pack pass (8 without cost) + 1
by the count pass, 28 written per finished episode, 20 per env of carry read
and 20 written.  hbm_floor_us is those bytes at 8 TB/s.  The repetitions reuse
one set of inputs: 11.8 MB at (65 536, 20) stays in the 256 MB Infinity Cache
(a warm-cache figure), 590 MB at (65 536, 1000) does not."""
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

HBM_BYTES_PER_S = 8.0e12


def torch_stats(reward, cost, done, carry, length):
    """The records and the running sums with torch ops (what a user writes)."""
    import torch
    K, B = reward.shape
    d = done != 0
    steps = torch.arange(K, device=reward.device)[:, None]
    last = torch.cummax(torch.where(d, steps, torch.full_like(steps, -1)), 0).values  # last end up to and at j
    prev = torch.cat([torch.full_like(last[:1], -1), last[:-1]], 0)  # ... before j
    idx = d.reshape(-1).nonzero()[:, 0]  # step-major, env-minor
    j, i = idx // B, idx % B
    p = prev[j, i]
    first = p < 0
    out = {"env": i.to(torch.int32), "step": j.to(torch.int32),
           "length": torch.where(first, length[i].long() + j + 1, j - p).to(torch.int32)}
    for col, v in enumerate((reward, cost)):
        cs = torch.cumsum(v.double(), 0)
        before = torch.where(first, -carry[i, col], cs[p.clamp(min=0), i])
        out["reward" if col == 0 else "cost"] = cs[j, i] - before
        at_last = cs[last[-1].clamp(min=0), torch.arange(B, device=v.device)]
        out["carry%d" % col] = torch.where(last[-1] < 0, cs[-1] + carry[:, col], cs[-1] - at_last)
    out["len"] = torch.where(last[-1] < 0, length.long() + K, K - 1 - last[-1]).to(torch.int32)
    return out


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


def measure(B, K, a):
    import torch

    from rcbf_amd import EpisodeStats, _lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    reward = torch.randn(K, B, device="cuda", generator=gen)
    cost = torch.rand(K, B, device="cuda", generator=gen)
    done = (torch.rand(K, B, device="cuda", generator=gen) < 1 / 300).to(torch.uint8)
    length = torch.randint(0, 299, (B,), device="cuda", generator=gen, dtype=torch.int32)
    carry = torch.randn(B, 2, device="cuda", generator=gen, dtype=torch.float64)
    traj = {"reward": reward, "cost": cost, "done": done}
    env = types.SimpleNamespace(num_envs=B, step_count=length)

    def stats():
        s = EpisodeStats(env)
        s.running()[0].copy_(carry)
        return s

    # the two device paths agree on these inputs (the torch one to rounding: it subtracts prefix sums)
    st = stats()
    rec = st.update(traj)
    n_ep = rec["n_episodes"]
    ref = torch_stats(reward, cost, done, carry, length)
    assert n_ep == ref["env"].numel() and all(torch.equal(rec[f], ref[f]) for f in ("env", "step", "length"))
    assert torch.equal(st.running()[1], ref["len"])
    rel = max(float(((rec[f] - ref[f]).abs() / (1 + ref[f].abs())).max()) if n_ep else 0.0 for f in ("reward", "cost"))
    rel = max(rel, float(((st.running()[0][:, 0] - ref["carry0"]).abs() / (1 + ref["carry0"].abs())).max()))
    assert rel < 1e-9, rel
    out = {"B": B, "K": K, "n_episodes": n_ep, "max_rel_diff_vs_torch": rel}

    lib = _lib.load()
    n_alloc = max(n_ep, 1)
    rec_i = torch.empty(3, n_alloc, dtype=torch.int32, device=dev)
    rec_f = torch.empty(2, n_alloc, dtype=torch.float64, device=dev)
    cnt = torch.empty(2, dtype=torch.int64, device=dev)
    scr = torch.empty(lib.rcbf_traj_episode_stats_scratch_bytes(B, K) // 8, dtype=torch.int64, device=dev)
    cout, lout = torch.empty_like(carry), torch.empty_like(length)
    p, stream = _lib.ptr, _lib.stream_of(dev)

    def call():
        rc = lib.rcbf_traj_episode_stats_f64(p(rec_i[0]), p(rec_i[1]), p(rec_i[2]), p(rec_f[0]), p(rec_f[1]), p(cnt),
                                             p(scr), B, K, B, p(reward), p(cost), p(done), p(carry), p(length),
                                             p(cout), p(lout), 1, n_alloc, stream)
        assert rc == 0

    def count_only():
        rc = lib.rcbf_traj_episode_stats_f64(None, None, None, None, None, p(cnt), p(scr), B, K, B, p(reward), p(cost),
                                             p(done), None, None, None, None, 1, 0, stream)
        assert rc == 0

    st = stats()
    call_us, count_us, update_us, torch_us = [], [], [], []
    for _ in range(a.rounds):  # alternating rounds
        call_us.append(timed(call, a.reps))
        count_us.append(timed(count_only, a.reps))
        update_us.append(timed(lambda: st.update(traj), a.reps))
        torch_us.append(timed(lambda: torch_stats(reward, cost, done, carry, length), a.reps))
    host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (reward, cost, done)]
    d2h = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for h, t in zip(host, (reward, cost, done)):
            h.copy_(t, non_blocking=True)
        torch.cuda.synchronize()
        d2h.append((time.perf_counter() - t0) * 1e6)

    def med(v):
        return sorted(v)[len(v) // 2]

    nbytes = K * B * 10 + 28 * n_ep + 40 * B
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    out.update({"call_us_rounds": [round(v, 1) for v in call_us], "count_us_rounds": [round(v, 1) for v in count_us],
                "update_us_rounds": [round(v, 1) for v in update_us],
                "torch_us_rounds": [round(v, 1) for v in torch_us], "d2h_us": [round(v) for v in d2h],
                "algorithmic_bytes": nbytes, "hbm_floor_us": round(floor_us, 2),
                "call_fraction_of_hbm_floor": round(floor_us / med(call_us), 3),
                "call_TB_per_s": round(nbytes / med(call_us) / 1e6, 3),
                "torch_over_call": round(med(torch_us) / med(call_us), 1),
                "d2h_over_call": round(med(d2h) / med(call_us), 1)})
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x20,65536x1000,64x1000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "exp_traj_stats.py measures on the GPU"
    for shape in a.shapes.split(","):
        B, K = (int(v) for v in shape.split("x"))
        measure(B, K, a)


if __name__ == "__main__":
    main()
