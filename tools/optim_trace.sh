# Launch counts of the optimizer side of a step, on a GPU:  bash tools/optim_trace.sh [reps] [output directory]
#   two rocprofv3 --kernel-trace --stats runs (no counters) per (parameter list, path) of tools/optim_bench.py --trace: the set-up alone
#   (--reps 0) and the set-up + reps calls; their difference is what the calls launched  -> <output directory>/kernel_stats.txt
#   (default output directory: build/optim_trace under the repository, which git ignores)
REPS=${1:-20}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${2:-$R/build/optim_trace}
mkdir -p $O
: > $O/kernel_stats.txt
cd /tmp && export TMPDIR=/tmp
for arch in x3d_s r2plus1d_18 resnet18_xprotonet resnet18_protopnet; do
  for mode in adam-torch adam-flat accum-none accum-torch accum-flat; do
    for reps in 0 $REPS; do
      rm -rf $O/run$reps
      timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $O/run$reps -o p -- python3 $R/tools/optim_bench.py --trace $mode --arch $arch --reps $reps > $O/run.log 2>&1
      rc=$?
      if [ $rc -ne 0 ]; then echo "$arch $mode --reps $reps: traced run failed with status $rc"; tail -5 $O/run.log; exit $rc; fi
    done
    echo "== $arch $mode ($REPS calls)" >> $O/kernel_stats.txt
    python3 $R/tools/optim_bench.py --stats-summary "$(find $O/run$REPS -name '*kernel_stats.csv' | head -1)" \
      --baseline "$(find $O/run0 -name '*kernel_stats.csv' | head -1)" --reps $REPS >> $O/kernel_stats.txt
  done
done
rm -rf $O/run0 $O/run$REPS $O/run.log
cat $O/kernel_stats.txt
