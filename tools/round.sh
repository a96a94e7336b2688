#!/bin/bash
# usage: tools/round.sh <tag> [cpu]  -- the round's measurement pass on one GPU box: the GPU parity suite; the bench line of
# every BASELINE config and of every wrench benchmark workload (with "cpu": the swgl CPU baseline beside EVERY one of them, one core
# and one process per core); the N > 1 path's world-1 self-test; rocprofv3 kernel stats of cfg2-5; HBM traffic (separate FETCH / WRITE
# passes) and SQ counters of cfg2 / cfg3 / cfg4 / cfg5.  Every bench line is a --full one.  Everything lands in $WRHIP_OUT/<tag>/
# (default out/<tag>/); copy what is to be judged to profiles/.
tag=$1; cpu=$2
export WRHIP_OUT=${WRHIP_OUT:-out}; out=$WRHIP_OUT/$tag
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p $out
(time timeout 1500 python -m pytest tests -m gpu -q 2>&1 | grep -v "RCCL\|HIP version\|ROCm version\|Hostname\|Librccl\|amdgpu.ids" | tail -15) > $out/gpu_tests.log 2>&1
cat $out/gpu_tests.log
# (the HBM counter passes first, and their summaries into profiles/ ON THE BOX: bench.py takes `traffic` from the newest summary there that was
# measured with these very kernel sources -- after a kernel edit the committed ones no longer match, and the lines below would carry null)
for w in cfg2 cfg3 cfg4 cfg5; do bash tools/pmc_hbm.sh ${tag}_pmc_hbm_$w $w > $out/pmc_hbm_$w.log 2>&1; cp $WRHIP_OUT/${tag}_pmc_hbm_$w.json profiles/ 2>/dev/null; done
nocpu="--no-cpu-baseline"; [ "$cpu" = cpu ] && nocpu=""
python bench.py --full --steps 20 --warmup 5 > $out/bench_cfg2.json 2> $out/bench_cfg2.err
for w in cfg1 cfg3 cfg4 cfg5; do
  python bench.py --full --workload $w --steps 50 --warmup 5 2>/dev/null | grep '"metric"' > $out/bench_$w.json
done
python bench.py --full --sharded --steps 20 --warmup 3 2>/dev/null | grep '"metric"' > $out/bench_sharded_world1_cfg5.json
for W in 2 4 8; do python bench.py --emulate-world $W --steps 20 --warmup 3 2>/dev/null | grep '"metric"' > $out/bench_emulate_world${W}_cfg5.json; done
for wl in aligned-gradient unaligned-gradient simple-batching large-boxshadow-ellipse large-boxshadow-ellipse-2 large-clip-rect transforms text-rendering many-images large-blur-radius many-box-shadows clip-clear overlapping-text-shadows; do
  python bench.py --full --workload $wl --steps 40 --warmup 5 $nocpu 2>/dev/null | grep '"metric"' > $out/bench_${wl}.json
done
for w in cfg2 cfg3 cfg4 cfg5; do
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$w -o r -- python bench.py --full --workload $w --steps 50 --warmup 5 --no-cpu-baseline > /dev/null 2>&1
  cp $out/prof_$w/r_kernel_stats.csv $out/${w}_kernel_stats.csv
  rm -rf $out/prof_$w
done
WORKLOADS="cfg2 cfg3 cfg4 cfg5" bash tools/sq.sh ${tag} > $out/sq.log 2>&1
grep -h '"metric"' $out/bench_*.json | python3 -c "
import sys, json
for l in sys.stdin:
    d = json.loads(l); r = d.get('roofline') or {}
    print(d['config']['workload'][:26], 'fps', d['value'], 'lat_ms', d.get('frame_latency_ms'), 'dom', r.get('kernel'), r.get('avg_launch_us'), 'frac', r.get('frac'), 'cpu', (d.get('cpu_baseline') or {}).get('value'), ((d.get('cpu_baseline') or {}).get('multi_process') or {}).get('value'))"
