#!/usr/bin/env python3
"""Table of the exposed chain tail of matvec_q8t_kernel from the JSON lines of scripts/probes/matvec_stamp_probe.hip.
    python scripts/matvec_chain_tail.py parent.jsonl new.jsonl [...]  > table.md
Per launch class and build: the time between the chip-wide last "products done" and the chip-wide last "result stored" (median over
the probe's launches, ns on the 100 MHz clock), the same per workgroup (median workgroup), the duration of the last chain (segment),
and the launch's span from the first workgroup's start to the last store.  Several files of one build are shown as a range."""
import collections, json, re, sys

rows = collections.defaultdict(lambda: collections.defaultdict(list))       # class -> build -> [record]
barrier = collections.defaultdict(list)
order = []
for f in sys.argv[1:]:
    for ln in open(f):
        if not ln.startswith("{"):
            continue
        d = json.loads(ln)
        build = re.sub(r"\d+$", "", d["build"])          # parent, parent2, ... are repeats of one build
        if d["class"] == "barrier_round":
            barrier[(build, d["waves"])].append(d["ns_per_round_median"])
            continue
        if d["class"] not in order:
            order.append(d["class"])
        rows[d["class"]][build].append(d)


def rng(v):
    return "%.0f" % v[0] if min(v) == max(v) else "%.0f–%.0f" % (min(v), max(v))


builds = sorted({b for c in rows.values() for b in c}, key=lambda b: (b != "parent", b))
print("| class | K | groups | workgroups | NPW | build | chip tail ns | workgroup tail ns | last chain ns | span ns |")
print("|---|---|---|---|---|---|---|---|---|---|")
for c in order:
    for b in builds:
        r = rows[c].get(b)
        if not r:
            continue
        print("| %s | %d | %d | %d | %d | %s | %s | %s | %s | %s |" % (c, r[0]["k"], r[0]["ng"], r[0]["wgs"], r[0]["npw"], b, rng([x["chip_tail_ns_median"] for x in r]),
              rng([x["wg_tail_ns_median"] for x in r]), rng([x["last_chain_ns_median"] for x in r]), rng([x["span_ns_median"] for x in r])))
print()
for (b, w), v in sorted(barrier.items()):
    print("barrier round, %d wavefronts per workgroup (%s): %s ns" % (w, b, rng(v)))
