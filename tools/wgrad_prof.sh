#!/bin/bash
# dev: per-kernel durations of tools/wgrad_bench.py (the host-side planning of an eager flush is longer than its kernels)
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD; OUT=$ROOT/gpurun_out; mkdir -p $OUT; export TMPDIR=/tmp
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/wgp -- python3 $ROOT/tools/wgrad_bench.py "$@" > $OUT/wgrad_prof.log 2>&1) || { tail -5 $OUT/wgrad_prof.log; exit 1; }
python - <<PY
import glob, sqlite3
db = glob.glob("$OUT/wgp/**/*.db", recursive=True)[0]
c = sqlite3.connect(db)
rows = c.execute("select name, start, end from kernels order by start").fetchall()
import collections
seq = [(n.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], (e - s) / 1e3) for n, s, e in rows if "wgrad" in n or "weightnorm" in n]
# 12 flushes per configuration (--kinds): print the last flush of each configuration
out, cur = [], []
for name, us in seq:
    cur.append((name, us))
    if "weightnorm" in name:
        out.append(cur); cur = []
for i in range(11, len(out), 12):
    print(" | ".join(f"{n[-28:]} {us:7.1f}" for n, us in out[i]), " total", round(sum(us for _, us in out[i]), 1))
    timed = out[i - 9:i + 1]                                     # the 10 timed flushes: mean and range per launch
    for k, (n, _) in enumerate(out[i]):
        v = [f[k][1] for f in timed if len(f) == len(out[i])]
        print(f"    {n[-28:]}  mean {sum(v) / len(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}  ({len(v)} launches)")
PY
rm -rf $OUT/wgp
