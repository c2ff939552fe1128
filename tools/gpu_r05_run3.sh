export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT; O=gpurun_out/r05_run3; mkdir -p $O
for i in 1 2; do python bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/bench_default_$i.json 2> $O/bench_default_$i.err; python - <<PY
import json
d=json.loads(open("$O/bench_default_$i.json").read().strip().splitlines()[-1])
w=d["workloads"]
print("run $i: dtu", round(d["value"],1), "| lego", w["lego"].get("fps"), w["lego"].get("latency_ms"), "| zju", w["zju"].get("fps"), w["zju"].get("latency_ms"), "| train", w["train"].get("ms_per_step"), "wall", w.get("wall_s"))
PY
done
timeout 900 python -m pytest tests/test_training.py tests/test_train_glue.py -m gpu -x -q 2>&1 | tail -3
python bench.py --train --no-perceptual --steps 20 --warmup 3 --no-live-pmc > $O/train_noperc.json 2> $O/train_noperc.err; python -c "
import json; t=json.loads(open('$O/train_noperc.json').read().strip().splitlines()[-1]); print('train noperc', round(t['ms_per_step'],3), 'ms/step')"
bash tools/gpu_train_stats.sh r05_run3/train --no-perceptual > $O/train_stats.log 2>&1; grep -E "launches per step|library kernels" $O/train_stats.log
