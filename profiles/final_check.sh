# Build, GPU tests, smoke() and one bench.py --full run of the tree as it stands; logs go to OUTDIR.
# usage: bash profiles/final_check.sh OUTDIR
set -eo pipefail   # a failed step ends the script, also inside a pipeline (smoke | cut)
OUT=${1:?usage: bash profiles/final_check.sh OUTDIR}
mkdir -p "$OUT"
timeout -k 10 900 python -c "import __graft_entry__ as g; g.build()" > "$OUT/final_build.log" 2>&1 || { tail -20 "$OUT/final_build.log"; exit 1; }
tail -1 "$OUT/final_build.log"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/final_gpu_tests.log" 2>&1 || { tail -40 "$OUT/final_gpu_tests.log"; exit 1; }
tail -1 "$OUT/final_gpu_tests.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | cut -c1-120
SECONDS=0
timeout -k 10 600 python bench.py --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err"
echo "bench wall seconds: $SECONDS"
python -c "
import json, sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], round(d['roofline']['frac'],4), d['sac_first_capture']['vector_steps'])" "$OUT/final_bench.json"
