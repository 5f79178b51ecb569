#!/bin/bash
# One GPU-box session: the -m gpu suite, smoke(), the headline bench, the cfg4 (bf16) line and the secondary benches.
#   bash tools/gpu_check.sh [<tag>]      (logs and JSON lines under $OUT_DIR/<tag>, default /tmp/gpu_check/<tag>)
tag=${1:-check}
cd "$(dirname "$0")/.."
out=${OUT_DIR:-/tmp/gpu_check}/$tag
mkdir -p $out
export TMPDIR=/tmp
timeout 1500 python -m pytest tests -q -m gpu --timeout 600 2>&1 | tail -15 | tee $out/tests.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -3 | tee $out/smoke.log
timeout 600 python bench.py --full > $out/bench.json 2> $out/bench.err; tail -c 400 $out/bench.json
timeout 300 python bench.py --full --config cfg4 --no-cpu-baseline --no-dense > $out/bench_cfg4.json 2> $out/bench_cfg4.err
timeout 300 python tools/bench_extra.py > $out/secondary.json 2> $out/secondary.err; cat $out/secondary.json
python - <<PY
import json
for n in ("bench", "bench_cfg4"):
    try:
        d = json.load(open("$out/%s.json" % n)); print(n, d["value"], d["ms_per_step"], d["dtype"], d["roofline"]["frac"])
    except Exception as e:
        print(n, "failed", e)
PY
