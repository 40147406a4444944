#!/bin/bash
# calc_view with a preset's formats compiled in against the parent build, on one box in one call.
#   scripts/view_presets_measure.sh PARENT.so [OUT_DIR] [counters|bench|all]
# PARENT.so = the library of the parent commit (unitygaussiansplatting_amd.build.build_variant on its sources); the change is the in-tree library.
# counters: one `rocprofv3 --pmc SQ_INSTS_VALU` pass and one `--kernel-trace --stats` pass of the driver's frames (one frame at a time), each build, each pass
#           a run of its own.   bench: plain `python bench.py` (the headline, two frames in flight), parent and change alternating, three each; then C3 and
#           the one-frame-at-a-time visible mode, two each.   scripts/view_presets_summary.py OUT_DIR turns the directory into profiles/view_presets_bench.json.
# Every step runs under its own time limit and the script stops at the first step that fails.
set -o pipefail
PARENT=${1:?parent library}; R=$(cd "$(dirname "$0")/.." && pwd); O=${2:-$R/view_presets_out}; WHAT=${3:-all}
mkdir -p $O; cd $R; export PYTHONPATH=$R
use() { if [ $1 = parent ]; then export GSPLAT_LIB=$PARENT; else unset GSPLAT_LIB; fi; }
if [ $WHAT = counters ] || [ $WHAT = all ]; then
  BENCH="python $R/bench.py --config C2 --sort-mode visible --steps 20 --warmup 5"
  for who in parent change; do
    use $who
    timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d $O/pmc_$who -- $BENCH > $O/pmc_$who.json 2> $O/pmc_$who.err || { tail -5 $O/pmc_$who.err; exit 1; }
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_$who -- $BENCH > $O/stats_$who.json 2> $O/stats_$who.err || { tail -5 $O/stats_$who.err; exit 1; }
  done
fi
run() {   # run <tag> <parent|change> <bench.py arguments...>
  local tag=$1 who=$2; shift 2
  use $who
  timeout -k 10 240 python $R/bench.py "$@" > $O/$tag.json 2> $O/$tag.err || { echo "FAILED $tag"; tail -5 $O/$tag.err; exit 1; }
  echo "$tag $(tail -1 $O/$tag.json | cut -c1-60)"
}
if [ $WHAT = bench ] || [ $WHAT = all ]; then
  for k in 1 2 3; do run headline_parent_$k parent; run headline_change_$k change; done
  for k in 1 2; do run c3_parent_$k parent --config C3; run c3_change_$k change --config C3; done
  for k in 1 2; do run visible_parent_$k parent --sort-mode visible; run visible_change_$k change --sort-mode visible; done
fi
unset GSPLAT_LIB
python $R/scripts/view_presets_summary.py $O
