#!/usr/bin/env python
"""Per-kernel MEDIAN duration from a rocprofv3 --kernel-trace csv (means carry the odd 2 ms outlier of a traced run):

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 bench.py --inflight 1 --no-secondary-legs ...
  python tools/trace_medians.py <dir>/**/*_kernel_trace.csv

Rows are sorted by launches x median; the last line sums that over the Winograd conv family (wino_conv3x3_*)."""
import csv
import sys
from collections import defaultdict

d = defaultdict(list)
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        d[r['Kernel_Name']].append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
rows = []
for k, v in d.items():
    v.sort()
    short = k.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')
    rows.append((len(v) * v[len(v) // 2], short, len(v), v[len(v) // 2], sum(v) / len(v)))
tot_w = 0.0
for tot, short, n, med, mean in sorted(rows, reverse=True):
    print(f'{short[:64]:64s} launches {n:5d}  median {med / 1e3:8.1f} us  mean {mean / 1e3:8.1f} us  launches x median {tot / 1e6:8.3f} ms')
    if 'wino_conv3x3' in short:
        tot_w += tot
print(f'wino_conv3x3 family: launches x median, summed: {tot_w / 1e6:.3f} ms over the trace')
