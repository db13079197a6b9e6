#!/bin/bash
# collect_fy_pmc.sh extended to the gather: rocprofv3 --pmc passes over k_fy_gather_select_multi in tools/exp/fy_bench at L = 10^6
# (build it with tools/exp/build.sh first), one counter per run, kernel trace only -- never combined with a sys / runtime trace --
# at each setting "n rot" of the gather's XCD subset (ACAV_GS_XCDS, ACAV_GS_XCD_ROT).  One iteration per launch: the table shows
# the median, the least and the most over the launches.  It goes to <out>/<prefix>_gs_xcd_pmc.txt.
#   tools/collect_gs_pmc.sh [out dir] [prefix] ["8 0" "4 1" ...]
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT=${1:-profiles/out}; P=${2:-r17}; shift 2
[ $# -gt 0 ] || set -- "8 0" "4 0" "4 1" "2 0" "1 0"
mkdir -p "$OUT"
[ -x tools/exp/fy_bench ] || { echo "tools/exp/fy_bench is missing: tools/exp/build.sh fy_bench"; exit 1; }
T="$OUT/${P}_gs_xcd_pmc.txt"
echo "# rocprofv3 --pmc <one counter> --kernel-trace, k_fy_gather_select_multi in tools/exp/fy_bench 1000000, per launch = per iteration" > "$T"
for S in "$@"; do
    set -- $S
    for C in TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum TCC_REQ_sum; do
        D="$OUT/pmc_gs_$1_$2_$C"
        rm -rf "$D"
        ACAV_GS_XCDS=$1 ACAV_GS_XCD_ROT=$2 timeout -k 10 300 rocprofv3 --pmc $C --kernel-trace --kernel-include-regex "k_fy_gather" \
            --output-format csv -d "$D" -o pmc -- tools/exp/fy_bench 1000000 > "$OUT/pmc_gs_$1_$2_$C.log" 2>&1
        rc=$?
        if [ $rc -ne 0 ]; then echo "rocprofv3 pass $C (ACAV_GS_XCDS=$1 ACAV_GS_XCD_ROT=$2) ended with $rc: stopping"; tail -5 "$OUT/pmc_gs_$1_$2_$C.log"; exit $rc; fi
        F=$(find "$D" -name "*counter_collection.csv" | head -1)
        [ -n "$F" ] || { echo "no csv for $C (ACAV_GS_XCDS=$1 ACAV_GS_XCD_ROT=$2)"; exit 1; }
        python3 - "$F" "ACAV_GS_XCDS=$1 ACAV_GS_XCD_ROT=$2" <<'PY' | tee -a "$T"
import csv, statistics, sys
rows = list(csv.DictReader(open(sys.argv[1])))
v = [float(r["Counter_Value"]) for r in rows]
print("%-34s %-20s launches %-5d median %9.0f  min %9.0f  max %9.0f" % (sys.argv[2], rows[0]["Counter_Name"], len(v), statistics.median(v), min(v), max(v)))
PY
        rm -rf "$D"
    done
done
