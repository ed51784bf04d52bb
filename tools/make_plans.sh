#!/bin/bash
# Run ON THE GPU BOX: time the launch plans of every workload bench.py measures into $OUT/plans_new/ (to be committed under
# computer-vision-shoplifting-detection_amd/plans/).  Shipped files are ignored while doing so (MI355_PLAN_DIR points at an empty directory).
cd "$GRAFT_REPO_ROOT"
export OUT=$(mkdir -p "${OUT:-tools_out}" && cd "${OUT:-tools_out}" && pwd)     # raw output, absolute: the plan variables below need it
mkdir -p $OUT/plans_new $OUT/empty_dir
rm -f $OUT/plans_new/*.plan
export MI355_PLAN_DIR=$OUT/empty_dir MI355_PLAN_CACHE=$OUT/plans_new
timeout -k 10 1100 python bench.py --full --steps 20 --warmup 5 > $OUT/make_plans_bench.json 2> $OUT/make_plans_bench.err || { tail -20 $OUT/make_plans_bench.err; exit 1; }
# the half=True headline form of config 5 at batch 16 as the rocprof collection runs it (chunk 16) is the same shape as the configs entry
ls $OUT/plans_new | wc -l
python - <<'PY'
import json, os
d = json.loads(open(os.environ["OUT"] + "/make_plans_bench.json").read().strip().splitlines()[-1])
print(d["value"], d["roofline"]["frac"], d["roofline"]["plan_source"], [(c["workload"], c["value"], c["roofline"]["frac"]) for c in d["configs"]], d["track_pipeline"])
PY
