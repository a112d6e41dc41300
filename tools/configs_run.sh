#!/bin/bash
# throughput of the other BASELINE configurations (information for DESIGN.md section 6; the headline is the default run) -> $OUT
OUT=${OUT:-evidence_out}
mkdir -p $OUT
python bench.py --full --no-cpu --mix --channels 4096 --tiles 24 --steps 100 | tee $OUT/bench_mix4096.json
python bench.py --full --no-cpu --channels 8192 --tiles 24 --steps 100 | tee $OUT/bench_8192x24.json
python bench.py --full --no-cpu --channels 4096 --tiles 96 --steps 50 | tee $OUT/bench_4096x96.json
