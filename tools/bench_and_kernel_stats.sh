#!/bin/bash
# Run on an MI355X; results land in $OUT (default: build/bench_stats/ of the repository).
# the full bench line (--full: every leg) + rocprofv3 kernel stats of the headline-only run
repo=$(cd "$(dirname "$0")/.." && pwd)
out=${OUT:-$repo/build/bench_stats}
mkdir -p "$out"
cd "$repo"
python bench.py --full > "$out/bench_default.json" 2> "$out/bench_default.err"
tail -c 2500 "$out/bench_default.json"
cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/prof
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/prof -o bench -- python "$repo/bench.py" > /tmp/prof_bench.json 2>/tmp/prof.err
cd "$repo"
f=$(find /tmp/prof -name "*.db" | head -1)
python - > "$out/kernel_stats.csv" <<PY
import sqlite3
db=sqlite3.connect("$f")
tot=db.execute("select sum(end-start) from kernels").fetchone()[0]
print("kernel,calls,total_ms,avg_us,min_us,max_us,pct")
for r in db.execute("select name,count(*),sum(end-start)/1e6,avg(end-start)/1e3,min(end-start)/1e3,max(end-start)/1e3,100.0*sum(end-start)/%d from kernels group by name order by 3 desc" % tot):
    print('"%s",%d,%.2f,%.1f,%.1f,%.1f,%.2f' % (r[0][:110],r[1],r[2],r[3],r[4],r[5],r[6]))
PY
# (last argument 3: layer3 chains of csrc/chain3.hip + layer1 conv front, round 6)
python tools/layer_report.py $f 9600 17 1 3 > "$out/layer_report.txt"
tail -1 /tmp/prof_bench.json | cut -c1-300
