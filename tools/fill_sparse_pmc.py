#!/usr/bin/env python3
"""Per-pass FETCH_SIZE / WRITE_SIZE of tools/micro/fill_sparse --pmc, from two
rocprofv3 --pmc runs (one counter each, no tracing).  The variant is in the kernel
name: k_sparse<non-temporal, 16-byte units per piece, dirty set, blocks per CU>.

usage: fill_sparse_pmc.py FETCH_DIR WRITE_DIR
"""
import csv, glob, os, statistics, sys


def load(d, counter):
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row["Counter_Name"] != counter:
                continue
            name = row["Kernel_Name"].split("(")[0].replace("void ", "")
            per.setdefault(name, []).append((int(row["Dispatch_Id"]), float(row["Counter_Value"]) * 1024.0))
    return per


fe, wr = load(sys.argv[1], "FETCH_SIZE"), load(sys.argv[2], "WRITE_SIZE")
print("kernel<NT, units per piece, dirty set, blocks/CU>: bytes per pass (median of the last 2 of 3), raw counters x 1024")
for k in sorted(set(fe) & set(wr)):
    f = statistics.median(v for _, v in sorted(fe[k])[-2:])
    w = statistics.median(v for _, v in sorted(wr[k])[-2:])
    print("%-28s FETCH_SIZE %8.1f MB  WRITE_SIZE %8.1f MB  (%d launches)" % (k, f / 1e6, w / 1e6, len(fe[k])))
