#!/bin/bash
# per-kernel device time of one dual-band streaks run (tools/bench_streaks.py, 1 timed step of STREAKS_PLANES planes,
# default 256 x 2048^2 uint16) from a rocprofv3 kernel trace: total, launches and share of every kernel class.
# STREAKS_ROUTE=march (with STREAKS_MAX_BATCH, default 32): the march route -- the log-space chain's kernels are counted too
# STREAKS_ARGS: further arguments of tools/bench_streaks.py, e.g. "--smoothing 1 --shading" (the options blend k_st_blendx)
set -o pipefail
PLANES=${STREAKS_PLANES:-256}
ROUTE=${STREAKS_ROUTE:-generic}
OUT=$(mktemp -d)
rocprofv3 --kernel-trace --output-format csv -d "$OUT" -- \
  python3 tools/bench_streaks.py --planes "$PLANES" --steps 1 --warmup 0 --route "$ROUTE" \
  --max-batch "${STREAKS_MAX_BATCH:-32}" ${STREAKS_ARGS:-} > /dev/null || exit $?
python3 - "$PLANES" "$OUT" "$ROUTE" <<'PY'
import collections, csv, glob, sys
tot, cnt = collections.Counter(), collections.Counter()
for f in glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if "k_st_" not in name and (sys.argv[3] == "generic" or "dsx::" not in name):
            continue
        key = name.replace("void ", "").replace("dsx::st::", "").replace("dsx::", "").replace("(anonymous namespace)::", "").split("(")[0]
        tot[key] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        cnt[key] += 1
planes = int(sys.argv[1])
all_ns = sum(tot.values())
print("kernel class                          launches   total ms   us/plane   share")
for k, v in tot.most_common():
    print("%-36s %9d %10.3f %10.2f %6.1f %%" % (k, cnt[k], v / 1e6, v / 1e3 / planes, 100.0 * v / all_ns))
print("%-36s %9d %10.3f %10.2f" % ("all", sum(cnt.values()), all_ns / 1e6, all_ns / 1e3 / planes))
PY
rc=$?
rm -rf "$OUT"
exit $rc
