#!/bin/bash
# A/B of the headline between two built trees on one GPU:
#   scripts/ab_bench.sh PARENT_TREE OUTDIR [VAR=value]
#                                               (from the root of the new tree)
# `python bench.py --gpus 1 --steps 200 --warmup 10` alternately in PARENT_TREE
# and here, five runs each, then twice here under VAR=value: the switch that
# takes the new build back to the parent's path (default VSA_TUNE=4, the
# candidate sort through rocPRIM; VSA_TUNE=16 for the walk of the planned
# search).  The two runs are named new_<value in lower case, letters and digits
# only>_1 and _2 (new_tune4_1, new_tune16_1).  Every run under a timeout of
# its own; the first run that fails ends the script.  OUTDIR gets the JSON
# line of every run (bench_line_<name>.json) and ab_bench.txt, one
# "name ms_per_step value" line per run made from those.
set -o pipefail
PARENT=$(cd "$1" && pwd) || exit 2
NEW=$PWD
mkdir -p "$2" || exit 2
OUT=$(cd "$2" && pwd)
VAR=${3:-VSA_TUNE=4}
# VSA_TUNE=4 -> tune4
TAG=$(printf '%s' "${VAR#VSA_}" | tr 'A-Z' 'a-z' | tr -cd 'a-z0-9')
: > "$OUT/ab_bench.txt"
run() { # tree name [VAR=value]
  (cd "$1" && timeout -k 10 200 env ${3:-VSA_AB=1} python bench.py --gpus 1 \
      --steps 200 --warmup 10 2> "$OUT/bench_$2.err" | tail -1 \
      > "$OUT/bench_line_$2.json") || return 1
  python -c "import json, sys; print(sys.argv[1], 'ms_per_step', '%.4f' % json.load(open(sys.argv[2]))['ms_per_step'])" \
      "$2" "$OUT/bench_line_$2.json" | tee -a "$OUT/ab_bench.txt" || return 1
  rm -f "$OUT/bench_$2.err"
}
run "$PARENT" parent_1 && run "$NEW" new_1 &&
run "$PARENT" parent_2 && run "$NEW" new_2 &&
run "$PARENT" parent_3 && run "$NEW" new_3 &&
run "$PARENT" parent_4 && run "$NEW" new_4 &&
run "$PARENT" parent_5 && run "$NEW" new_5 &&
run "$NEW" "new_${TAG}_1" "$VAR" && run "$NEW" "new_${TAG}_2" "$VAR"
