"""What recording a trajectory costs: one process, one library (RCBF_HIP_LIB, or
the product's), one workload; prints one JSON line per plan form and length.

  traj      fused trajectory plan, every field recorded, run(copy_back=False)
  per_step  the per-step plan (fused=False), no trajectory: K dispatches
  fused     the fused plan, no trajectory

--old: the library is a build of the commit before trajectory plans (it has no
rcbf_aql_safe_step_traj_plan): the binding is not asked for that entry point
and `traj` is not measured.  Each figure is the median over `reps` runs of the
host clock around plan.run(sync_hip=False), which returns when the K steps
have completed; B = 65 536, bench.py's start states and action pool.  Driven
by scripts/ab_traj.sh, which alternates the two libraries."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "sac-rcbf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def compare_dumps(d1, d2):
    import numpy as np
    n1, n2 = sorted(os.listdir(d1)), sorted(os.listdir(d2))
    same = n1 == n2 and bool(n1)
    for n in n1 if n1 == n2 else []:
        x, y = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        eq = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        print(n, x.dtype, x.shape, "bit-equal" if eq else "DIFFERENT")
        same = same and eq
    print("dumps bit-equal" if same else f"dumps DIFFER ({n1} / {n2})")
    sys.exit(0 if same else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="cars", choices=["cars", "u5"])
    ap.add_argument("--old", action="store_true")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--forms", default=None, help="comma list of traj,per_step,fused (default: by --old)")
    ap.add_argument("--code-object", default=None,
                    help="the step kernels' code object (default: librcbf_steps.co beside the library); a variant "
                         "build's NAME.co, whose NAME_traj.co is loaded with it")
    ap.add_argument("--lacks", default="", help="comma list of entry points the library (RCBF_HIP_LIB) does not "
                                                "have yet: the binding is not asked for them")
    ap.add_argument("--lib-tag", default=None, help="the `lib` field of the output lines (default: new / old)")
    ap.add_argument("--compare-dumps", nargs=2, metavar="DIR", default=None,
                    help="compare two bench.py --dump-outputs directories bit for bit, and exit")
    a = ap.parse_args()
    if a.compare_dumps:
        return compare_dumps(*a.compare_dumps)
    import torch

    from rcbf_amd import _lib
    if a.old:
        _lib.SIGNATURES.pop("rcbf_aql_safe_step_traj_plan")
    for name in filter(None, a.lacks.split(",")):
        _lib.SIGNATURES.pop(name)
    import bench
    from rcbf_amd.aql import AqlQueue
    from rcbf_amd.diff_cbf_qp import CBFQPLayer
    from rcbf_amd.envs import BatchedSimulatedCarsEnv, BatchedUnicycleEnv

    class Args:
        cuda = True

    dev = torch.device("cuda", 0)
    B = a.batch
    forms = a.forms.split(",") if a.forms else (["per_step", "fused"] if a.old else ["traj", "fused"])
    q = AqlQueue(dev, code_object=a.code_object)
    for K, reps in ((20, 5000), (1000, 150)):
        for form in forms:
            if a.env == "cars":
                env, name = BatchedSimulatedCarsEnv(B, device=dev, seed=1234), "SimulatedCars"
            else:
                env, name = BatchedUnicycleEnv(B, device=dev, seed=1234,
                                               hazards_locations=bench.unicycle_hazards(5)), "Unicycle"
            layer = CBFQPLayer(env, Args(), gamma_b=20.0)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(5)
            bench.init_states(env, gen, name)
            pool = [(torch.rand(B, env.n_u, device="cuda", generator=gen) * 2 - 1).contiguous() for _ in range(7)]
            o = env.make_outputs()
            kw = {"traj": {"trajectory": True}, "per_step": {"fused": False}, "fused": {}}[form]
            plan = q.safe_step_plan(env, pool, layer, steps=K, outputs=o, **kw)
            run = (lambda: plan.run(sync_hip=False, copy_back=False)) if form == "traj" else \
                (lambda: plan.run(sync_hip=False))
            torch.cuda.synchronize()
            for _ in range(max(3, reps // 20)):
                run()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter_ns()
                run()
                ts.append(time.perf_counter_ns() - t0)
            ts.sort()
            env.check_failures()
            print(json.dumps({"lib": a.lib_tag or ("old" if a.old else "new"), "env": a.env, "form": form, "K": K, "B": B,
                              "dispatches": plan.dispatches, "reps": reps,
                              "kernel": "" if "rcbf_aql_plan_form" not in _lib.SIGNATURES else plan.form,
                              "us_per_step_median": round(ts[len(ts) // 2] / 1e3 / K, 4),
                              "us_per_step_p10": round(ts[len(ts) // 10] / 1e3 / K, 4),
                              "us_per_step_p90": round(ts[9 * len(ts) // 10] / 1e3 / K, 4)}), flush=True)
            plan.free()
            del plan, env, layer, o
    q.close()


if __name__ == "__main__":
    main()
