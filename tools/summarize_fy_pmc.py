"""One table row per (setting, counter, position kernel) from rocprofv3 --pmc passes over tools/exp/fy_bench (one counter per
pass, kernel trace only): the median over the launches of each kernel, divided by the FY_GROUP = 16 iterations of a launch.
argv: a title line, then  label=path/to/counter_collection.csv ...  (the counter's name is read from the file)."""
import csv
import re
import statistics
import sys

print("# " + sys.argv[1])
print("# median over the launches of each kernel, divided by 16 iterations per launch: per iteration")
for arg in sys.argv[2:]:
    label, path = arg.rsplit("=", 1)
    per = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")).split("<")[0].strip()
        per.setdefault((r["Counter_Name"], name), []).append(float(r["Counter_Value"]))
    for (ctr, name), vals in sorted(per.items()):
        print(f"{label:<24} {ctr:<20} {name:<20} launches {len(vals):<4} per iteration {statistics.median(vals) / 16:10.0f}")
