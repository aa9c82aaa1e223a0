# Whole GPU suite (one process, per-test timeouts), then the default bench line without the CPU leg.
# usage: bash tools/gpu_suite.sh [extra pytest args]
O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 1000 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread --durations=12 -p no:cacheprovider "$@" > $O/suite.log 2>&1
rc=$?
tail -18 $O/suite.log
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $O/bench.json 2> $O/bench.err || exit $?
python3 -c "
import json; d=json.loads(open('$O/bench.json').read().strip().splitlines()[-1])
print('value', d['value'], 'ms/step', d['ms_per_step'], 'ratio', d['config']['compression_ratio']); print(d['kernel_ms_per_step']); print(d['roofline_decode'])"
