#!/bin/bash
# A/B of in-flight sub-batches per GPU (contexts/streams) and stream gates on
# the default bench workload.   usage (on the box): bash tools/streams_ab.sh "ARGS" ["ARGS" ...]
#   e.g. bash tools/streams_ab.sh "--streams 2 --gate 2,4" "--streams 3 --gate 2,4"
set -e
O=${MSGPU_OUT:-bench_out}; mkdir -p "$O"
for a in "$@"; do
  timeout -k 10 200 python bench.py --full --no-cpu --points= $a > $O/st.json 2>/dev/null
  python3 -c "
import json;d=json.load(open('$O/st.json'));print('$a', d['ms_per_step'], d['value'], d['checked']['all_ok'])"
done
