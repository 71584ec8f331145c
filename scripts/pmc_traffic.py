"""HBM traffic per launch of the convolution family from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) of the bench command:
    python scripts/pmc_traffic.py <fetch counter_collection.csv> <write counter_collection.csv> <dtype> <source text> > profiles/r03_pmc_traffic.json
FETCH_SIZE x 2 (gfx950 tallies 128-byte requests as 64: MI355X_MICROARCH.md, HBM section) + WRITE_SIZE, both in KiB, summed over every dispatch
whose kernel name contains "conv" and divided by the number of such dispatches.  Also prints the per-kernel table to stderr."""
import collections
import csv
import json
import re
import sys


def load(path, counter):
    per = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == counter:
            per[r["Kernel_Name"]].append(float(r["Counter_Value"]))
    return per


def short(name):
    m = re.search(r"(conv\w*_k|conv3x3_c64_k|splitk_reduce\w*|stem_\w+_k|bn_\w+_k|channel_reduce_k|adam_\w+_k|maxpool\w+_k|head_\w+_k|weight_prep_k)", name)
    return m.group(1) if m else name[:48]


fetch, write = load(sys.argv[1], "FETCH_SIZE"), load(sys.argv[2], "WRITE_SIZE")
tot, n = 0.0, 0
rows = collections.defaultdict(lambda: [0, 0.0, 0.0])
for k, v in fetch.items():
    rows[short(k)][0] += len(v)
    rows[short(k)][1] += sum(v) * 2 * 1024
for k, v in write.items():
    rows[short(k)][2] += sum(v) * 1024
for k, (cnt, fb, wb) in sorted(rows.items(), key=lambda kv: -(kv[1][1] + kv[1][2])):
    print("%-28s n=%5d  fetched %9.1f MB/launch  written %9.1f MB/launch" % (k, cnt, fb / max(cnt, 1) / 1e6, wb / max(cnt, 1) / 1e6), file=sys.stderr)
    if "conv" in k:
        tot += fb + wb
        n += cnt
json.dump({sys.argv[3]: {"traffic_bytes_per_launch": round(tot / max(n, 1)),
                         "kernel": "convolution family, average over the %d conv dispatches of the profiled command" % n,
                         "source": sys.argv[4]}}, sys.stdout, indent=1)
