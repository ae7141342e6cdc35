# A/B of the cars fused plan's straight-line loop (rcbf::k_safe_steps_fast, csrc/rcbf_safe_steps_fast.hpp) against
# the commit before it, by scripts/ab_carry.sh's protocol: one GPU session, the libraries alternating, 5 rounds:
# this tree ("new"), a built checkout of the parent commit ("old", whose library lacks rcbf_aql_plan_form), and,
# where they were built, the stage variants build/variants/librcbf_NAME.co with NAME_fast.co beside it
# (python __graft_entry__.py variant NAME -DRCBF_FAST_PAIR=0 [-DRCBF_FAST_AHEAD2=0]).  Legs (scripts/exp_traj_ab.py,
# B = 65 536, 20 and 1 000 steps): the cars plain fused plan, and the unicycle's at k = 5 as the control (its
# kernels did not change).  Then bench.py's driver form and its default form with --dump-outputs from both trees,
# compared bit for bit, and the table of the process medians.
# Usage: [RCBF_AB_OUT=OUT] [RCBF_AB_VARIANTS="NAME .."] bash scripts/ab_fast.sh TAG [PARENT_TREE]
cd "$(dirname "$0")/.."; R=$PWD; O=${RCBF_AB_OUT:-bench_out}; case $O in /*) ;; *) O=$R/$O;; esac; O=$O/$1
P=${2:-build/parent_tree}; mkdir -p $O
V=$R/$P/sac-rcbf_amd/rcbf_amd/librcbf_hip.so
[ -f $V ] || { echo "no parent build at $V"; exit 1; }
for r in 1 2 3 4 5; do
  for w in cars u5; do
    timeout -k 10 150 python scripts/exp_traj_ab.py --env $w --forms fused >> $O/new_$w.jsonl 2>> $O/err.log || { tail -5 $O/err.log; exit 1; }
    RCBF_HIP_LIB=$V timeout -k 10 150 python scripts/exp_traj_ab.py --env $w --forms fused --lib-tag old \
      --lacks rcbf_aql_plan_form >> $O/old_$w.jsonl 2>> $O/err.log || { tail -5 $O/err.log; exit 1; }
  done
  for n in $RCBF_AB_VARIANTS; do
    timeout -k 10 150 python scripts/exp_traj_ab.py --env cars --forms fused --lib-tag $n \
      --code-object build/variants/librcbf_$n.co >> $O/${n}_cars.jsonl 2>> $O/err.log || { tail -5 $O/err.log; exit 1; }
  done
  echo "round $r done"
done
for form in driver default; do
  a=""; [ $form = driver ] && a="--gpus 1 --steps 20 --warmup 5"
  timeout -k 10 300 python bench.py $a --dump-outputs $O/dump_${form}_new > $O/bench_${form}_new.log 2>&1 || { tail -5 $O/bench_${form}_new.log; exit 1; }
  (cd $P && timeout -k 10 300 python bench.py $a --dump-outputs $O/dump_${form}_old > $O/bench_${form}_old.log 2>&1) || { tail -5 $O/bench_${form}_old.log; exit 1; }
  python scripts/exp_traj_ab.py --compare-dumps $O/dump_${form}_new $O/dump_${form}_old | tee $O/dump_compare_$form.txt || exit 1
  tail -1 $O/bench_${form}_new.log | cut -c1-400; tail -1 $O/bench_${form}_old.log | cut -c1-400
done
rm -rf $O/dump_*_new $O/dump_*_old
python - $O <<'EOF' | tee $O/table.txt
import glob, json, os, sys
rows = {}
for p in sorted(glob.glob(os.path.join(sys.argv[1], "*.jsonl"))):
    for ln in open(p):
        r = json.loads(ln)
        rows.setdefault((r["env"], r["form"], r["K"], r["lib"], r.get("kernel", "")), []).append(r["us_per_step_median"])
for k in sorted(rows):
    v = sorted(rows[k])
    print("%-5s %-6s K=%-5d %-5s %-10s medians %s  median %.4f  min-max %.4f-%.4f" % (*k, v, v[len(v) // 2], v[0], v[-1]))
EOF
