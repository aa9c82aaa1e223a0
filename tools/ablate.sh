#!/bin/bash
# Kernel-time / ratio comparisons of diagnostic library builds (never shipped). Args: tags of
# sample-s3-hybrid-cache_amd/build/diag/lib_<tag>.so ("base" = the shipped library).
O=${OUT:-bench_out}/abl
mkdir -p $O
for t in "$@"; do
  lib=$PWD/sample-s3-hybrid-cache_amd/build/diag/lib_$t.so
  [ "$t" = base ] && lib=$PWD/sample-s3-hybrid-cache_amd/libs3hc_lz4.so
  S3HC_LIB_PATH=$lib timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 5 --warmup 1 > $O/$t.log 2>&1 || { echo "$t failed"; tail -3 $O/$t.log; exit 1; }
  python -c "import json;d=json.loads(open('$O/$t.log').read().strip().splitlines()[-1]);print('$t', d['value'], d['config']['compression_ratio'], d['kernel_ms_per_step'])"
done
