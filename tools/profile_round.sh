#!/bin/bash
# Run on the GPU box (tools/gpu.sh -- 'bash tools/profile_round.sh TAG OUTDIR'): the default bench, the same step under
# rocprofv3 kernel stats, three separate PMC passes (never combined with other trace domains), the exact-arithmetic
# bench, the mean-field iteration (k_compat_softmax) under kernel stats + PMC, and the regime sweep.
# OUTDIR (relative to the repository root) receives the logs and traces.
# Condense afterwards with tools/save_profiles.py TAG prof_TAG prof_TAG_exact pmc_TAG OUTDIR.
set -o pipefail
tag=${1:-r01_final}
R=$GRAFT_REPO_ROOT
out=${2:?usage: profile_round.sh TAG OUTDIR}
OUT=$R/$out
mkdir -p $OUT
python $R/bench.py --full > $OUT/bench_final.log 2>$OUT/bench_final.err || exit 1
cd /tmp && export TMPDIR=/tmp
# the profiled command is the headline step only: the regime sweep and the mean-field extras launch the same kernels
# on other lattices / other shapes and would blur the per-kernel averages
Q="--no-cpu-baseline --no-regimes --no-mean-field"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -- python3 $R/bench.py $Q > $OUT/bench_final_prof.log 2>&1 || exit 1
for c in "FETCH_SIZE" "WRITE_SIZE" "TCC_HIT_sum TCC_MISS_sum"; do
  n=$(echo $c | cut -d" " -f1)
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/pmc_${tag}_$n -- python3 $R/bench.py --steps 3 --warmup 1 $Q > $OUT/pmc_${tag}_$n.log 2>&1 || exit 1
done
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${tag}_exact -- python3 $R/bench.py $Q --exact > $OUT/bench_final_exact.log 2>&1 || exit 1
# mean-field iteration: filter - Q, then the fused compatibility product + softmax (k_compat_softmax)
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${tag}_mf -- python3 $R/bench.py --full --no-cpu-baseline --no-regimes --no-small-image --steps 5 > $OUT/bench_final_mf.log 2>&1 || exit 1
for c in "FETCH_SIZE" "WRITE_SIZE"; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/pmc_${tag}_mf_$c -- python3 $R/bench.py --full --no-cpu-baseline --no-regimes --no-small-image --steps 2 --warmup 1 > $OUT/pmc_${tag}_mf_$c.log 2>&1 || exit 1
done
cd $R && python tools/regimes.py --workloads c3,c2 --out $out/regimes_$tag.json > $out/regimes_$tag.log 2>&1 || exit 1
grep "^{" $OUT/bench_final.log | cut -c1-200
