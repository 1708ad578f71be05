#!/bin/bash
# builds scan_geom_ab: the product scan in several variants (one object each)
set -e
out=$(realpath -m "${1:-/tmp/scan_geom_ab}")
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
cd "$(dirname "$0")"
b() { hipcc --offload-arch=gfx950 -O3 -std=c++17 -Dzc=zc_$1 -DSCAN_ENTRY=scan_v_$1 $2 -c scan_variant.hip -o $tmp/sv_$1.o; }
# (round 5 also measured 4 x 4 waves with lists of 64 / 48 entries: r05_scan_geom_ab.txt)
# and 2 x 4 waves with 256-byte rounds (-DZC_ROUND_CFG=256): r05_scan_geom_ab2.txt
# and 2 KiB lane spans (-DZC_LSPAN_CFG=2048): r05_scan_geom_ab3/4.txt
# and 3 x 4 waves (-DZC_SCAN_WG_PER_CU_CFG=3): r05_scan_geom_ab4.txt
# and two ring slots / one workgroup with two / the contiguous probe (-DZC_SCAN_SLOTS_CFG=2,
# -DZC_SCAN_WG_PER_CU_CFG=1, -DZC_CONTIG_PROBE_CFG=1): r05_scan_geom_ab5.txt
# and the round-6 hand-off priority variants (-DZC_SCAN_PRIO_CFG=1/2/3): r06_scan_prio_ab.txt (no gain; default 0)
# now: the static stride and the re-priming of every half (the parent) against
# the claimed wave-tiles and the even lanes' rolled-on state, each alone and
# both (the product), and the parent and the product with stamps
old="-DZC_SCAN_CLAIM_CFG=0 -DZC_SCAN_ROLL_CFG=0"
pids=()
b parent "$old" & pids+=($!)
b claim "-DZC_SCAN_CLAIM_CFG=1 -DZC_SCAN_ROLL_CFG=0" & pids+=($!)
b roll "-DZC_SCAN_CLAIM_CFG=0 -DZC_SCAN_ROLL_CFG=1" & pids+=($!)
b prod "" & pids+=($!)
b parent_stamp "$old -DZC_SCAN_STAMP_CFG=1" & pids+=($!)
b prod_stamp "-DZC_SCAN_STAMP_CFG=1" & pids+=($!)
hipcc --offload-arch=gfx950 -O3 -std=c++17 -c scan_geom_ab.hip -o $tmp/scan_geom_ab.o & pids+=($!)
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -o $out $tmp/scan_geom_ab.o $tmp/sv_parent.o $tmp/sv_claim.o $tmp/sv_roll.o $tmp/sv_prod.o \
  $tmp/sv_parent_stamp.o $tmp/sv_prod_stamp.o
