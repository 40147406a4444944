"""scripts/view_presets_measure.sh's output directory -> one JSON document (profiles/view_presets_bench.json): the counter pass, the kernel stats and
every bench line of the parent build and of the change, and whether the gain counts by the rule of the measurement: every run of the change below every
run of the parent, by more than the parent's own min-to-max spread.

    python scripts/view_presets_summary.py OUT_DIR [profiles/view_presets_bench.json]"""
import collections
import csv
import glob
import json
import os
import sys


def last_json(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def counters(out_dir, who):
    per = collections.defaultdict(lambda: collections.defaultdict(float))      # kernel -> dispatch -> counter summed over its rows
    for f in glob.glob(os.path.join(out_dir, "pmc_" + who, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == "SQ_INSTS_VALU" and "calc_view" in row["Kernel_Name"]:
                per[row["Kernel_Name"]][row["Dispatch_Id"]] += float(row["Counter_Value"])
    return {k: {"launches": len(v), "mean": round(sum(v.values()) / len(v)), "min": round(min(v.values())), "max": round(max(v.values()))} for k, v in per.items()}


def stats(out_dir, who):
    st = {}
    for f in glob.glob(os.path.join(out_dir, "stats_" + who, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "calc_view" in row["Name"]:
                st[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                   "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return st


def bench(out_dir, tag):
    res = {}
    for who in ("parent", "change"):
        runs = []
        for f in sorted(glob.glob(os.path.join(out_dir, f"{tag}_{who}_*.json"))):
            j = last_json(f)
            runs.append({"run": os.path.basename(f)[:-5], "ms_per_step": j["ms_per_step"], "value": j["value"], "sort_mode": j.get("config", {}).get("sort_mode")})
        res[who] = runs
    p, c = [r["ms_per_step"] for r in res["parent"]], [r["ms_per_step"] for r in res["change"]]
    if p and c:
        spread = max(p) - min(p)
        res["parent_spread_ms"] = round(spread, 4)
        res["every_change_run_below_every_parent_run"] = max(c) < min(p)
        res["margin_ms"] = round(min(p) - max(c), 4)                           # the smallest gap between a parent run and a change run
        res["gain_counts"] = max(c) < min(p) and (min(p) - max(c)) > spread
        res["median_gain_ms"] = round(sorted(p)[len(p) // 2] - sorted(c)[len(c) // 2], 4)                 # (upper median; information, not part of the rule)
        res["not_slower_beyond_spread"] = max(c) <= max(p) + spread
    return res


def main():
    out_dir = sys.argv[1]
    doc = {"what": "calc_view with a creator preset's formats compiled in (change) against the parent build; one box, one call; scripts/view_presets_measure.sh",
           "counter_pass": {"command": "rocprofv3 --pmc SQ_INSTS_VALU -- python bench.py --config C2 --sort-mode visible --steps 20 --warmup 5",
                            "valu_wave_insts_per_launch": {w: counters(out_dir, w) for w in ("parent", "change")}},
           "kernel_stats": {"command": "rocprofv3 --kernel-trace --stats -- python bench.py --config C2 --sort-mode visible --steps 20 --warmup 5",
                            "calc_view_us_per_launch": {w: stats(out_dir, w) for w in ("parent", "change")}},
           "headline_C2_visible_in_flight": dict(command="python bench.py", **bench(out_dir, "headline")),
           "C3": dict(command="python bench.py --config C3", **bench(out_dir, "c3")),
           "C2_visible_one_frame_at_a_time": dict(command="python bench.py --sort-mode visible", **bench(out_dir, "visible"))}
    text = json.dumps(doc, indent=1)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
