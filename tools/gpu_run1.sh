#!/bin/bash
# GPU box: the -m gpu test suite, then (unless the tests were killed) the default bench line.  Logs under $OUT/.
OUT=${OUT:-tool_out}                 # where the logs and traces go
mkdir -p $OUT
timeout -k 10 ${T_TESTS:-700} python -m pytest tests -m gpu -q -s -p no:cacheprovider ${PYTEST_ARGS} > $OUT/tests.log 2>&1
rc=$?
echo "pytest exit $rc"; tail -n 25 $OUT/tests.log | cut -c1-300
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "tests were killed: not starting the bench"; exit $rc; fi
timeout -k 10 ${T_BENCH:-420} python bench.py --steps ${STEPS:-10} --warmup 3 --full ${BENCH_ARGS} > $OUT/bench.json 2> $OUT/bench.err
rb=$?
echo "bench exit $rb"; cat $OUT/bench.json | cut -c1-2500; grep -v Warning $OUT/bench.err | tail -n 12 | cut -c1-300
exit $(( rc != 0 ? rc : rb ))
