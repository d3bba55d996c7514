#!/bin/bash
# full GPU suite + smoke + extended fuzz of the loss path + the two bench invocations (--full, and the plain headline run)
# Every GPU step runs under a time limit of its own; the first step that fails, aborts or runs out of time ends the script.
OUT=${OUT:-validate_out}
mkdir -p $OUT
stop() { echo "stopped at $1 (exit status $2)"; exit "$2"; }
timeout -k 10 1500 python -m pytest tests -q -m gpu --maxfail=20 -p no:cacheprovider > $OUT/validate_pytest_full.log 2>&1; rc=$?
tail -6 $OUT/validate_pytest_full.log; [ $rc -eq 0 ] || stop pytest $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/validate_smoke.log 2>&1; rc=$?
tail -2 $OUT/validate_smoke.log; [ $rc -eq 0 ] || stop smoke $rc
timeout -k 10 600 python tools/extended_fuzz.py 24 500 loss > $OUT/validate_fuzz.log 2>&1; rc=$?
echo "fuzz rc=$rc"; tail -3 $OUT/validate_fuzz.log; [ $rc -eq 0 ] || stop fuzz $rc
timeout -k 10 600 python bench.py --full > $OUT/validate_bench.json 2> $OUT/validate_bench.err || stop bench $?
timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/validate_bench_driver.json 2> $OUT/validate_bench_driver.err || stop bench-driver $?
python - $OUT/validate_bench.json $OUT/validate_bench_driver.json <<'PY'
import json, sys
for f in sys.argv[1:]:
    try:
        r = json.loads(open(f).read().strip().splitlines()[-1])
        rf = r.get('roofline', {})          # roofline and extras: --full only
        print(f, 'us/step %.2f' % (r['ms_per_step'] * 1e3), 'frac', rf.get('frac'), 'sol_us', rf.get('sol_us'),
              {k: (round(v['us_per_step'], 2) if isinstance(v, dict) and 'us_per_step' in v else None) for k, v in r.get('extras', {}).items() if k.startswith('n')})
    except Exception as e:
        print(f, 'FAILED', e)
PY
