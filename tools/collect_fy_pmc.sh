#!/bin/bash
# rocprofv3 --pmc passes over the position kernels ALONE (tools/exp/fy_bench at L = 10^6; build it with tools/exp/build.sh first),
# with the 3-D grids of the tile and resolve kernels (ACAV_FY_XCD_AFFINE=0) and with the XCD-affine 1-D grids (=1): one counter per
# run, kernel trace only -- never combined with a sys / runtime trace.  The table goes to <out>/<prefix>_mi_xcd_affine_pmc.txt.
#   tools/collect_fy_pmc.sh [out dir] [prefix]
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT=${1:-profiles/out}; P=${2:-r15}
mkdir -p "$OUT"
[ -x tools/exp/fy_bench ] || { echo "tools/exp/fy_bench is missing: tools/exp/build.sh fy_bench"; exit 1; }
ARGS=()
for A in 0 1; do
    for C in TCC_REQ_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum; do
        D="$OUT/pmc_fy_${A}_$C"
        rm -rf "$D"
        ACAV_FY_XCD_AFFINE=$A timeout -k 10 300 rocprofv3 --pmc $C --kernel-trace --kernel-include-regex "k_fy_(part|tile|resolve)" \
            --output-format csv -d "$D" -o pmc -- tools/exp/fy_bench 1000000 > "$OUT/pmc_fy_${A}_$C.log" 2>&1
        rc=$?
        if [ $rc -ne 0 ]; then echo "rocprofv3 pass $C (affine $A) ended with $rc: stopping"; tail -5 "$OUT/pmc_fy_${A}_$C.log"; exit $rc; fi
        F=$(find "$D" -name "*counter_collection.csv" | head -1)
        [ -n "$F" ] || { echo "no csv for $C (affine $A)"; exit 1; }
        cp "$F" "$OUT/${P}_fy_pmc_${A}_${C}.csv"
        rm -rf "$D"
        ARGS+=("ACAV_FY_XCD_AFFINE=$A=$OUT/${P}_fy_pmc_${A}_${C}.csv")
    done
done
python tools/summarize_fy_pmc.py "rocprofv3 --pmc <one counter> --kernel-trace, tools/exp/fy_bench 1000000 (ACAV_FY_XCD_AFFINE=0: 3-D grids, 1: one XCD per iteration)" \
    "${ARGS[@]}" | tee "$OUT/${P}_mi_xcd_affine_pmc.txt"
