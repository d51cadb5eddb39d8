#!/bin/bash
# Runs tools/gather_policy_probe.hip: one timing run (no profiler), then rocprofv3 counter passes, each a run of its own with
# one hot-table size and no tracing beside the counters.  Every step has its own time limit and the script stops at the first
# step that fails.
#   bash tools/gather_policy_probe.sh [OUTDIR]          (default build/gather_policy_probe_out)
# Results: OUTDIR/timing.txt (the probe's table and JSON line), OUTDIR/counters.txt (per hot table and variant: L2 hit rate, L2
# requests per gather, fabric bytes per gather = FETCH_SIZE x 2 on gfx950).
OUT=${1:-build/gather_policy_probe_out}
BIN=build/gather_policy_probe
mkdir -p "$OUT" build || exit 1
if [ ! -x $BIN ] || [ tools/gather_policy_probe.hip -nt $BIN ]; then
  hipcc -O3 --offload-arch=gfx950 tools/gather_policy_probe.hip -o $BIN || exit 1
fi
export TMPDIR=/tmp
timeout -k 10 240 $BIN --rounds 7 --reps 3 > "$OUT/timing.txt" 2>&1 || { echo "timing run failed"; tail -5 "$OUT/timing.txt"; exit 1; }
cat "$OUT/timing.txt"
for hot in 2 128; do
  i=0
  for pass in "TCC_HIT_sum TCC_MISS_sum" "FETCH_SIZE"; do
    i=$((i+1))
    timeout -k 10 240 rocprofv3 --pmc $pass --output-format csv -d "$OUT/hot${hot}_pass$i" -o run -- $BIN --rounds 1 --reps 1 --hot-mib $hot \
      > "$OUT/hot${hot}_pass$i.out" 2> "$OUT/hot${hot}_pass$i.err" || { echo "counter pass $i (hot table $hot MiB) failed"; tail -5 "$OUT/hot${hot}_pass$i.err"; exit 1; }
  done
done
python3 - "$OUT" <<'PY' | tee "$OUT/counters.txt"
import collections
import csv
import glob
import json
import os
import re
import sys

out = sys.argv[1]
names = {(0, 1): "hot_only", (0, 0): "cold_only_plain", (1, 0): "cold_only_nt"}
for every in (4, 8):
    for pol, tag in enumerate(("plain", "nt", "sc1", "sc0sc1")):
        names[(pol, every)] = "hot1of%d_cold_%s" % (every, tag)
names[(4, 4)], names[(5, 4)] = "hot1of4_cold_plain_builtin", "hot1of4_cold_nt_builtin"
gathers = json.loads(open(os.path.join(out, "timing.txt")).read().strip().splitlines()[-1])["gathers_per_launch"]
for hot in (2, 128):
    per = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(out, "hot%d_pass*" % hot, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_probe<(\d+), *(\d+)>", r["Kernel_Name"])
            if m:
                per[(int(m.group(1)), int(m.group(2)))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("hot table %d MiB (the last dispatch of each kernel; the first warms up)" % hot)
    print("%-28s %10s %14s %16s" % ("variant", "L2 hit", "L2 req/gather", "fabric B/gather"))
    for key, name in names.items():
        c = per.get(key)
        if not c:
            continue
        hit, miss, fetch = c["TCC_HIT_sum"][-1], c["TCC_MISS_sum"][-1], c["FETCH_SIZE"][-1]
        print("%-28s %10.4f %14.3f %16.1f" % (name, hit / (hit + miss), (hit + miss) / gathers, fetch * 1024 * 2 / gathers))
PY
