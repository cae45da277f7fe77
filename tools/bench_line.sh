#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
# the full line (every leg) and a summary of it: bash tools/bench_line.sh OUTDIR -> OUTDIR/bench_default.json, OUTDIR/err.txt
out=${1:?usage: tools/bench_line.sh OUTDIR}
mkdir -p "$out"
python bench.py --full 2>"$out/err.txt" | grep '^{' > "$out/bench_default.json"
python - "$out/bench_default.json" <<'PY'
import json, sys; d=json.load(open(sys.argv[1])); r=d['roofline']
print('value %.4g ms_per_step %.4f avg_launch_ms %.5f frac %.3f traffic %s hbm_frac %.3f' % (d['value'], d['ms_per_step'], r['avg_launch_ms'], r['frac'], r['traffic'], r['hbm_frac']))
print('sustained', {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d['sustained'].items() if k not in ('note', 'per_second')})
for k, v in d['end_to_end'].items(): print(' e2e', k, v if isinstance(v, str) else {a: (round(b, 3) if isinstance(b, float) else b) for a, b in v.items() if a != 'workload'})
for c in d['configs']: print(' %-11s %.4g spread %.3f launch %.2f us traffic %s parity %s' % (c['name'], c['value'], c['run_spread'], c['avg_launch_us'], c.get('traffic_bytes_per_point_sweep'), c['parity_bitwise']))
PY
