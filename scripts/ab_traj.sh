# A/B of trajectory plans against the commit before them, in one GPU session, the two libraries alternating,
# 5 pairs: this tree ("new": the fused trajectory plan with every field recorded, and the plain fused plan)
# against a built checkout of the parent commit ("old": its per-step plan, until now the only way to get at
# per-step values, and its plain fused plan).  Cars and the unicycle at k = 5, B = 65 536, 20 and 1 000 steps
# (scripts/exp_traj_ab.py; one JSON line per figure in OUT/TAG/{new,old}_{cars,u5}.jsonl).  Then
# bench.py's driver form with --dump-outputs from both trees, compared bit for bit.
# Usage: [RCBF_AB_OUT=OUT] bash scripts/ab_traj.sh TAG [PARENT_TREE]
#   OUT: output directory, default bench_out (relative to the repository); PARENT_TREE: default build/parent_tree, built
cd "$(dirname "$0")/.."; R=$PWD; O=${RCBF_AB_OUT:-bench_out}; case $O in /*) ;; *) O=$R/$O;; esac; O=$O/$1
P=${2:-build/parent_tree}; mkdir -p $O
V=$P/sac-rcbf_amd/rcbf_amd/librcbf_hip.so
[ -f $V ] || { echo "no parent build at $V"; exit 1; }
for r in 1 2 3 4 5; do for w in cars u5; do
  timeout -k 10 150 python scripts/exp_traj_ab.py --env $w >> $O/new_$w.jsonl 2>> $O/err.log || exit 1
  RCBF_HIP_LIB=$V timeout -k 10 150 python scripts/exp_traj_ab.py --env $w --old >> $O/old_$w.jsonl 2>> $O/err.log || exit 1
done; done
a="--gpus 1 --steps 20 --warmup 5"
timeout -k 10 200 python bench.py $a --dump-outputs $O/dump_new > $O/bench_new.log 2>&1 || exit 1
(cd $P && timeout -k 10 200 python bench.py $a --dump-outputs $O/dump_old > $O/bench_old.log 2>&1) || exit 1
python scripts/exp_traj_ab.py --compare-dumps $O/dump_new $O/dump_old | tee $O/dump_compare.txt
