#!/bin/bash
# Decode kernel time of two builds on the bench frame (4032x3008 q50,
# tools/kbench.py), the two libraries alternated, N runs of each per decoder
# arrangement (fused: k_decode_idct, reported as huff_decode; split:
# k_huff_decode + k_dequant_idct):
#   tools/dec_ab.sh <parent libmyyuv_hip.so> <new libmyyuv_hip.so> [N=5]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
PAR=$1; NEW=$2; N=${3:-5}
for dec in fused split; do
  for i in $(seq 1 $N); do
    for tag in parent new; do
      lib=$NEW; [ $tag = parent ] && lib=$PAR
      echo "== $dec $tag run $i"
      MYYUV_DECODER=$dec MYYUV_HIP_LIB=$lib timeout -k 10 120 python3 $R/tools/kbench.py 20 2>&1 |
        grep -E "rc=|huff_decode|dequant" | sed "s#$R/##" || exit 1
    done
  done
done
