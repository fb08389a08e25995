"""Per-class counter means of the bottleneck 3x3 kernels from rocprofv3 --pmc passes.

    python tools/pmc_conv3x3_nchw.py DIR [DIR ...] > summary.json

Each DIR holds one pass (run_counter_collection.csv; --pmc alone, no tracing) of
tools/bench_conv3x3_nchw.py --iters 2 --reps 1 --sides ....  Launches of the NCHW Winograd
kernels (every form) and of MIOpen's f2x3 Winograd kernel are grouped by kernel and grid size,
which together name the class and the form.  SQ_WAVE_CYCLES, SQ_WAIT_* and SQ_ACTIVE_INST_*
count in units of 4 cycles, SQ_VALU_MFMA_BUSY_CYCLES in cycles; the derived shares are of the
summed wave lifetime (pmc_conv3x3.py's conventions)."""
import collections
import csv
import json
import os
import re
import sys

QUAD = ('SQ_WAVE_CYCLES', 'SQ_WAIT_ANY', 'SQ_WAIT_INST_ANY', 'SQ_WAIT_INST_LDS', 'SQ_ACTIVE_INST_ANY',
        'SQ_ACTIVE_INST_LDS', 'SQ_ACTIVE_INST_VALU', 'SQ_ACTIVE_INST_VMEM')
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for d in sys.argv[1:]:
    for r in csv.DictReader(open(os.path.join(d, 'run_counter_collection.csv'))):
        name = r['Kernel_Name']
        m = re.search(r'conv3x3_nchw_\w+_kernel(<[^>]*>)?', name)
        if m:
            key = m.group(0)
        elif 'f2x3_stride1' in name:
            key = 'miopen f2x3_stride1'
        else:
            continue
        acc[(key, int(r['Grid_Size']), int(r['Workgroup_Size']))][r['Counter_Name']].append(float(r['Counter_Value']))
out = {}
for (key, grid, wg) in sorted(acc):
    a = acc[(key, grid, wg)]
    c = {k: sum(v) / len(v) for k, v in a.items()}
    row = {'launches': len(next(iter(a.values()))), 'counters': {k: round(v) for k, v in sorted(c.items())}}
    if 'SQ_WAVE_CYCLES' in c and 'SQ_WAVES' in c and c['SQ_WAVES'] > 0:
        life = 4.0 * c['SQ_WAVE_CYCLES']
        row['wave_cycles_per_wave'] = round(life / c['SQ_WAVES'])
        row['share_of_wave_lifetime'] = {k: round((4.0 if k in QUAD else 1.0) * v / life, 3) for k, v in sorted(c.items())
                                         if k != 'SQ_WAVE_CYCLES' and (k in QUAD or k == 'SQ_VALU_MFMA_BUSY_CYCLES')}
    out['{} grid {} wg {}'.format(key, grid, wg)] = row
print('{\n' + ',\n'.join(' {}: {}'.format(json.dumps(k), json.dumps(v)) for k, v in out.items()) + '\n}')
