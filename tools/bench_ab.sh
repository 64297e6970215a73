# bench.py --full under several environment settings (short runs, no CPU baseline): value / ms_per_step /
# decode step. Usage: OUT_DIR=... bash tools/bench_ab.sh ENV...
set -o pipefail
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:?set OUT_DIR to the directory the bench line goes to}
for e in "$@"; do
  env $e timeout -k 10 200 python3 $R/bench.py --full --steps ${BAB_STEPS:-3} --warmup 1 --no-cpu-baseline > $O/bab.json 2> $O/bab.err || { tail -5 $O/bab.err; exit 1; }
  python3 -c "
import json,sys; d=json.load(open('$O/bab.json'))
print('$e', 'value', d['value'], 'ms/step', d['ms_per_step'], 'decode_ms', d['decode_step_roofline']['ms_per_decode_step'], 'codec_ms', d['codec_roofline']['ms_per_batch'], 'att_us', round(d['kernels'].get('att_persist',{}).get('avg_us',0),2), 'b1_us', d.get('batch1',{}).get('decode_step_us'))"
done
