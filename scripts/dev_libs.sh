# dev: the headline bench on several builds of the library (A/B of dev knobs): bash scripts/dev_libs.sh dev/libA.so dev/libB.so ...
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mktemp -d)
for L in "$@"; do
  HANK_HIP_LIB=$R/$L timeout -k 10 200 python $R/bench.py --full --no-extra --no-cpu-baseline > $O/ab.json 2> $O/ab.err || { echo "$L: failed"; tail -3 $O/ab.err; continue; }
  python - "$L" <<PY
import json, sys
d = json.loads(open("$O/ab.json").read().strip().splitlines()[-1])
print(sys.argv[1], round(d["value"]), d["sweeps_ms"], flush=True)
PY
done
rm -rf "$O"
