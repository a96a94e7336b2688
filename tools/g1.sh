out=${WRHIP_OUT:-out}/r06_h
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p $out
for pin in 0 1 0 1; do
if [ $pin = 0 ]; then export WRHIP_BENCH_NO_PIN=1; else unset WRHIP_BENCH_NO_PIN; fi
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | grep '"metric"' > $out/b.json
python3 -c "
import json
d = json.load(open('$out/b.json')); r = d.get('roofline') or {}
print('cfg2 pin $pin', d.get('host_affinity'), 'fps', d['value'], 'regions', d['timed_regions_ms'], 'host', d.get('host'), 'busy', d.get('gpu_busy_frac'))"
done
uptime
