#!/bin/bash
# One event per context ("Stream ordering") against the parent build, on one box in one call: the method of view_presets_measure.sh.
#   scripts/stream_order_measure.sh PARENT.so [OUT_DIR] [RUNS]
# PARENT.so = the library of the parent commit (built from its sources with the same command); the change is the in-tree library.
# Plain `python bench.py`, parent and change alternating, RUNS (default 3) each, for the headline (two frames in flight: a lane crosses to its owner's
# target and back every frame), --sort-mode visible and --config C3.  Every step runs under its own time limit and the script stops at the first step
# that fails.  scripts/stream_order_summary.py OUT_DIR turns the directory into profiles/stream_order_bench.json.
set -o pipefail
PARENT=${1:?parent library}; R=$(cd "$(dirname "$0")/.." && pwd); O=${2:-$R/stream_order_out}; RUNS=${3:-3}
mkdir -p $O; cd $R; export PYTHONPATH=$R
run() {   # run <tag> <parent|change> <bench.py arguments...>
  local tag=$1 who=$2; shift 2
  if [ $who = parent ]; then export GSPLAT_LIB=$PARENT; else unset GSPLAT_LIB; fi
  timeout -k 10 240 python $R/bench.py "$@" > $O/$tag.json 2> $O/$tag.err || { echo "FAILED $tag"; tail -5 $O/$tag.err; exit 1; }
  echo "$tag $(tail -1 $O/$tag.json | cut -c1-60)"
}
for k in $(seq $RUNS); do run headline_parent_$k parent; run headline_change_$k change; done
for k in $(seq $RUNS); do run visible_parent_$k parent --sort-mode visible; run visible_change_$k change --sort-mode visible; done
for k in $(seq $RUNS); do run c3_parent_$k parent --config C3; run c3_change_$k change --config C3; done
unset GSPLAT_LIB
python $R/scripts/stream_order_summary.py $O
