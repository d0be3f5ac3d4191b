#!/bin/bash
# usage: scripts/pmc.sh <tag> "<counters>"   (on the GPU box; one --pmc pass per call, results under $LFR_PROF_OUT, default prof_out/)
set -e
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${LFR_PROF_OUT:-$R/prof_out}; mkdir -p $OUT
cd /tmp; export TMPDIR=/tmp
tag=$1; shift
rocprofv3 --pmc $1 --kernel-trace --output-format csv -d $OUT/pmc_$tag -o pmc -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/pmc_$tag.log 2>&1 || true
python - <<PY
import csv, collections, glob
f = glob.glob("$OUT/pmc_$tag/*counter_collection.csv")
agg = collections.defaultdict(lambda: collections.defaultdict(float)); cnt = collections.Counter()
for row in csv.DictReader(open(f[0])):
    k = row["Kernel_Name"][:60]
    agg[k][row["Counter_Name"]] += float(row["Counter_Value"])
    cnt[(k, row["Counter_Name"])] += 1
for k, d in agg.items():
    if "solve" not in k: continue
    print(k)
    for c, v in sorted(d.items()):
        print("   %-28s %16.0f per-dispatch" % (c, v / cnt[(k, c)]))
PY
