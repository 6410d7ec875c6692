#!/bin/bash
# FETCH_SIZE / WRITE_SIZE of the kernels of a training step (scripts/bench_train.py, 8 steps): the bytes the training forward
# FETCHES are its weight stream missing the L2.
#   bash scripts/pmc_train_fetch.sh <out dir>
set -u
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${1:?usage: bash scripts/pmc_train_fetch.sh <out dir>}
mkdir -p $OUT
for c in ${PMC_COUNTERS:-FETCH_SIZE WRITE_SIZE}; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/default_$c -o p -- python scripts/bench_train.py --steps 8 --warmup 2 ${BENCH_ARGS:-} > $OUT/default_$c.log 2>&1
done
python - "$OUT" <<'PY'
import csv, glob, sys, collections
out = sys.argv[1]
for c in __import__("os").environ.get("PMC_COUNTERS", "FETCH_SIZE WRITE_SIZE").split():
    files = glob.glob(f"{out}/default_{c}/**/*counter_collection.csv", recursive=True)
    if not files:
        continue
    acc, n = collections.defaultdict(float), collections.Counter()
    for row in csv.DictReader(open(files[0])):
        if row.get("Counter_Name") == c:
            k = row["Kernel_Name"].split("(")[0][-60:]
            acc[k] += float(row["Counter_Value"]); n[k] += 1
    top = sorted(acc.items(), key=lambda kv: -kv[1])[:8]
    print(c, "per launch (KiB for *_SIZE, counts otherwise):", {k: round(v / n[k], 1) for k, v in top}, "launches:", {k: n[k] for k, _ in top})
PY
find $OUT -name "*.csv" -size +1M -delete
