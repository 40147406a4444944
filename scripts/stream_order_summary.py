"""scripts/stream_order_measure.sh's output directory -> one JSON document (profiles/stream_order_bench.json): every bench line of the parent build and of
the change, and the verdict by the rule of the measurement -- a host-only change has no mechanism to cost more than run-to-run noise, so for each
configuration the change's median ms per frame may exceed the parent's median by no more than the parent's own spread (max - min over its runs).

    python scripts/stream_order_summary.py OUT_DIR [profiles/stream_order_bench.json]"""
import glob
import json
import os
import statistics
import sys


def bench(out_dir, tag):
    res = {}
    for who in ("parent", "change"):
        res[who] = []
        for f in sorted(glob.glob(os.path.join(out_dir, f"{tag}_{who}_*.json"))):
            j = json.loads(open(f).read().strip().splitlines()[-1])
            res[who].append({"run": os.path.basename(f)[:-5], "ms_per_step": j["ms_per_step"], "value": j["value"]})
    p, c = [r["ms_per_step"] for r in res["parent"]], [r["ms_per_step"] for r in res["change"]]
    if len(p) >= 3 and len(c) >= 3:
        res["parent_median_ms"], res["change_median_ms"] = round(statistics.median(p), 4), round(statistics.median(c), 4)
        res["parent_spread_ms"] = round(max(p) - min(p), 4)
        res["change_over_parent_ms"] = round(statistics.median(c) - statistics.median(p), 4)
        res["within_margin"] = statistics.median(c) - statistics.median(p) <= max(p) - min(p)
    return res


def main():
    out_dir = sys.argv[1]
    doc = {"what": "one event per context and gs::signal_to for every stream-to-stream edge (change) against the parent build; one box, one call, "
                   "parent and change alternating; scripts/stream_order_measure.sh",
           "rule": "per configuration: median(change) - median(parent) <= max(parent) - min(parent), ms per frame",
           "headline_C2_visible_in_flight": dict(command="python bench.py", **bench(out_dir, "headline")),
           "C2_visible_one_frame_at_a_time": dict(command="python bench.py --sort-mode visible", **bench(out_dir, "visible")),
           "C3": dict(command="python bench.py --config C3", **bench(out_dir, "c3"))}
    doc["verdict"] = "within the margin in every configuration" if all(doc[k].get("within_margin") for k in doc if isinstance(doc[k], dict)) \
        else "NOT within the margin (or fewer than three runs) in: " + ", ".join(k for k in doc if isinstance(doc[k], dict) and not doc[k].get("within_margin"))
    text = json.dumps(doc, indent=1)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
