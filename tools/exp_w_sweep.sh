T=$(mktemp -d)
for cfg in "RH_DX_W=2" "RH_DX_W=8" "RH_LIN_W=4" "RH_LIN_W=4 RH_DX_W=2"; do
  env $cfg python bench.py --full --no-cpu-baseline > $T/sw.json 2> $T/sw.err || { echo "$cfg failed"; tail -3 $T/sw.err; continue; }
  python -c "
import json; d=json.load(open('$T/sw.json')); print('$cfg', round(d['value'],1), round(d['ms_per_step'],2), {k:round(v['isolated_ms_per_step'],2) for k,v in d['roofline']['kernels'].items()})"
done
