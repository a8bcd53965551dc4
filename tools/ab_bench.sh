#!/bin/bash
# A/B of two builds of the library on one box: tools/ab_bench.sh <rounds> <lib A> <lib B> [bench.py arguments]
R=$1; A=$2; B=$3; shift 3
for r in $(seq $R); do for L in $A $B; do
    DL_LIB_PATH=$PWD/$L python bench.py --full "$@" 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
legs = {leg['id']: leg for leg in d.get('other_configs', []) if isinstance(leg, dict) and 'id' in leg}    # the line's legs (bench.py: other_configs); cfg4 = 'configs[3]-bao-xi'
bao = legs.get('configs[3]-bao-xi', {})
print('$L'.split('/')[-2:], 'us/step %.2f' % (1e3 * d['ms_per_step']), 'kernels', d.get('kernel_us'), 'cfg5', round(d.get('config5_strong', {}).get('us_per_update', 0), 1),
      'cfg4 us/step', round(1e3 * bao['ms_per_step'], 2) if bao.get('ms_per_step') else None, 'theory kernel', bao.get('kernel_us'))"
done; done
