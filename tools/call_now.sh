# scratch: the command of the last gpurun call of the round (gpu suite + smoke + three default bench lines at the final commit)
cd $GRAFT_REPO_ROOT
OUT=${OUT:-$(mktemp -d)}; mkdir -p $OUT; echo "outputs in $OUT"
timeout 1500 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.log 2>&1; tail -2 $OUT/pytest_gpu.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
for i in 1 2 3; do python bench.py --full > $OUT/bench_$i.json 2> $OUT/err_$i; python -c "
import json; d=json.loads(open('$OUT/bench_$i.json').read().strip().splitlines()[-1]); print(round(d['value']), round(d['ms_per_step'],3), d['parity_checked']['ok'], d['extra']['timed_steps']['host_thread_waits_ms_per_step'])"; done
