#!/bin/bash
# The measurements of profiles/live_notes.md section 2 in ONE call on one GPU: tools/live_ab.sh PARENT.so NEW.so [REPS]
# PARENT.so: libsonde_mi355.so built from the parent commit (git worktree add ../parent HEAD~1 && make -C ../parent/sdrpp_radiosonde_amd/csrc),
# NEW.so: this tree's.  The tuner's unchanged case is timed in alternating processes (parent, new, parent, ...), as tools/ab_bench.sh
# does for bench.py; then the idle-slot cost and the live receiver with this tree's library.  Every step has its own time limit and
# the first one that fails ends the script.
set -o pipefail
A=${1:?parent library}; B=${2:?new library}; REPS=${3:-3}
cd "$(dirname "$0")/.."
for rep in $(seq 1 $REPS); do
  for lib in "$A" "$B"; do
    SONDE_MI355_LIB=$(realpath "$lib") timeout -k 10 120 python tools/live_measure.py tuner | tail -1 || exit $?
  done
done
SONDE_MI355_LIB=$(realpath "$B") timeout -k 10 120 python tools/live_measure.py idle | tail -1 || exit $?
SONDE_MI355_LIB=$(realpath "$B") timeout -k 10 300 python tools/live_measure.py live | tail -1 || exit $?
