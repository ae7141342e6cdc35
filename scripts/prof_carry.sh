# rocprofv3 passes of bench.py's driver command (--gpus 1 --steps 20 --warmup 5) and its default command, for
# the parent commit's built checkout and this tree in one GPU session: a kernel trace, then two SQ counter
# passes, every pass a run of its own (no tracing beside the counters), each under its own time limit; the
# session stops at the first pass that fails.  Prints the rows of the timed kernel, k_safe_steps<0, 1, 256>
# (means per dispatch: scripts/pmc_sq.py; the trace: scripts/trace_summary.py); the raw csv stay in OUT/TAG.
# RCBF_PROF_KERN_BRANCH: the timed kernel's name on this tree's side where it is another (r16:
# "k_safe_steps_fast<256>").
# Usage: [RCBF_AB_OUT=OUT] [RCBF_PROF_KERN_BRANCH=NAME] bash scripts/prof_carry.sh TAG [PARENT_TREE]
cd "$(dirname "$0")/.."; R=$PWD; O=${RCBF_AB_OUT:-bench_out}; case $O in /*) ;; *) O=$R/$O;; esac; O=$O/$1
P=${2:-build/parent_tree}; mkdir -p $O
[ -f $P/sac-rcbf_amd/rcbf_amd/librcbf_hip.so ] || { echo "no parent build at $P"; exit 1; }
KERN="k_safe_steps<0, 1, 256>"
KERN_BRANCH=${RCBF_PROF_KERN_BRANCH:-$KERN}
C1="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES"
C2="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS"
for form in driver default; do
  a=""; [ $form = driver ] && a="--gpus 1 --steps 20 --warmup 5"
  for side in parent branch; do
    T=$R; [ $side = parent ] && T=$P
    K=$KERN_BRANCH; [ $side = parent ] && K=$KERN
    d=$O/${form}_$side
    (cd $T && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $d/trace -o run -- \
       python bench.py $a > $d.trace.log 2>&1) || { echo "$form $side: trace failed"; exit 1; }
    (cd $T && timeout -k 10 300 rocprofv3 --pmc $C1 --output-format csv -d $d/pmc1 -o run -- \
       python bench.py $a > $d.pmc1.log 2>&1) || { echo "$form $side: pmc1 failed"; exit 1; }
    (cd $T && timeout -k 10 300 rocprofv3 --pmc $C2 --output-format csv -d $d/pmc2 -o run -- \
       python bench.py $a > $d.pmc2.log 2>&1) || { echo "$form $side: pmc2 failed"; exit 1; }
    echo "== $form $side"
    python scripts/trace_summary.py "$(find $d/trace -name '*kernel_trace.csv' | head -1)" "$K"
    for p in pmc1 pmc2; do python scripts/pmc_sq.py "$(find $d/$p -name '*counter_collection.csv' | head -1)" "$K"; done
  done
done
