"""Average each PMC counter per kernel over a rocprofv3 --pmc output directory.
    python scripts/summarize_pmc.py DIR [substring]
A kernel launched with more than one grid size (a script that runs several shapes through the same kernels) gets
one block per grid size; `substring` keeps only the kernels whose name holds it."""
import collections
import csv
import glob
import sys

rows = []
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
only = sys.argv[2] if len(sys.argv) > 2 else ""
grids = collections.defaultdict(set)
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for r in rows:
    name = r.get("Kernel_Name", "?")
    if only not in name:
        continue
    short = name.replace("(anonymous namespace)::", "").split("(")[0][:90]
    grid = r.get("Grid_Size", "?")
    grids[short].add(grid)
    acc[(short, grid)][r["Counter_Name"]].append(float(r["Counter_Value"]))
for (k, grid), cs in acc.items():
    print(k if len(grids[k]) == 1 else f"{k}  [grid {grid}]")
    for c, v in sorted(cs.items()):
        print(f"   {c:28s} {sum(v)/len(v):18.10g}   (n={len(v)})")
