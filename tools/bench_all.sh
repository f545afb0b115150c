#!/usr/bin/env bash
# One `bench.py --full` line per BASELINE config into $OUT/<tag>_<workload>.json.log (copied to profiles/ afterwards).
# usage: [OUT=dir] tools/bench_all.sh <tag>
TAG="${1:-rXX}"
OUT="${OUT:-logs}"
mkdir -p "${OUT}"
for wl in cfg4_10Mx100M_24chrom cfg2_sparse_1Mx1M_1chrom cfg2_dense_1Mx1M_1chrom cfg3_semi_1Mx10M_24chrom cfg3_anti_1Mx10M_24chrom cfg3_count_1Mx10M_24chrom cfg5_nearest_10Mx10M_24chrom; do
  timeout -k 10 400 python3 bench.py --workload "$wl" --steps 10 --warmup 3 --full > "${OUT}/${TAG}_${wl}.json.log" 2> "${OUT}/${TAG}_${wl}.err"
  echo "$wl rc=$?"; tail -c 700 "${OUT}/${TAG}_${wl}.json.log"; echo
done
