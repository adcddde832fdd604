# input-stage kernels: their tests, the u8 input bench and the bench's hbm rows.  usage: run_dyn.sh <output directory>
out=${1:?usage: run_dyn.sh <output directory>}
mkdir -p $out
timeout -k 10 300 python -m pytest tests/test_kernels_gpu.py -x -q -k "dynimg or goal" > $out/t.log 2>&1; echo rc=$?; tail -3 $out/t.log
timeout -k 10 120 python scripts/dev/u8_input_bench.py 2>&1 | tail -1
timeout -k 10 300 python bench.py --full --steps 30 --warmup 8 --skip-cpu --skip-other-configs --skip-input-pipeline --skip-inference --skip-dp-one-rank > $out/bench.json 2> $out/bench.err; echo bench rc=$?
python -c "
import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], d['ms_per_step'], d['step_ms']); [print(r) for r in d['hbm']]" $out/bench.json
