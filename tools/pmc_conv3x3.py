"""Per-launch-shape counter means of conv3x3_bias_act_wino_kernel from rocprofv3 --pmc passes.

    python tools/pmc_conv3x3.py DIR [DIR ...] > summary.json

Each DIR holds one pass (run_counter_collection.csv) of tools/bench_conv3x3.py --fused-only.
Launches are grouped by grid size (327680 threads = P2 alone, 81920 = P3, 24576 = P4, 8192 = P5,
2048 = P6, 444416 / 442368 = the RPN / FPN multi-level launches).  SQ_WAVE_CYCLES, SQ_WAIT_* and
SQ_ACTIVE_INST_* count in units of 4 cycles, SQ_VALU_MFMA_BUSY_CYCLES in cycles; the derived
shares are of the summed wave lifetime."""
import collections
import csv
import json
import os
import sys

QUAD = ('SQ_WAVE_CYCLES', 'SQ_WAIT_ANY', 'SQ_WAIT_INST_ANY', 'SQ_WAIT_INST_LDS', 'SQ_ACTIVE_INST_ANY',
        'SQ_ACTIVE_INST_LDS', 'SQ_ACTIVE_INST_VALU', 'SQ_ACTIVE_INST_VMEM')
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for d in sys.argv[1:]:
    for r in csv.DictReader(open(os.path.join(d, 'run_counter_collection.csv'))):
        if 'conv3x3_bias_act_wino' in r['Kernel_Name']:
            acc[int(r['Grid_Size'])][r['Counter_Name']].append(float(r['Counter_Value']))
out = {}
for grid in sorted(acc, reverse=True):
    c = {k: sum(v) / len(v) for k, v in acc[grid].items()}
    row = {'launches': len(next(iter(acc[grid].values()))), 'counters': {k: round(v) for k, v in sorted(c.items())}}
    if 'SQ_WAVE_CYCLES' in c:
        life = 4.0 * c['SQ_WAVE_CYCLES']
        row['wave_cycles_per_wave'] = round(life / (grid / 64))
        row['share_of_wave_lifetime'] = {k: round((4.0 if k in QUAD else 1.0) * v / life, 3)
                                         for k, v in sorted(c.items())
                                         if k != 'SQ_WAVE_CYCLES' and (k in QUAD or k == 'SQ_VALU_MFMA_BUSY_CYCLES')}
    out[str(grid)] = row
# one line per launch shape
print('{\n' + ',\n'.join(' {}: {}'.format(json.dumps(k), json.dumps(v)) for k, v in out.items()) + '\n}')
