DT=${1:-f32}
run() { label=$1; shift
  env "$@" python bench.py --full --dtype $DT --steps 150 --warmup 3 --no-cpu-baseline --no-side-leg --no-other-configs 2>/dev/null | python -c "
import json,sys
r=json.loads([l for l in sys.stdin if l.startswith('{')][-1])
print('%-52s %8.2f samples/s  %7.3f ms/step  loss_ok=%s' % ('$label', r['value'], r['ms_per_step'], r['config'].get('loss_check',{}).get('ok')))"
}
for rep in 1 2 3; do
  run "$DT stride-2 input gradient: four launches" RCF_S2_DGRAD_ONE_LAUNCH=0
  run "$DT stride-2 input gradient: one launch (default)" RCF_X=1
done
