"""The planning span of each update in a rocprofv3 kernel trace of bench.py: from the end of the rollout's last
k_env_step to the start of the update's first k_ppo_loss, with the dispatches and the GPU-busy time inside it, and the
update's whole dispatch count.  python scripts/plan_span.py <trace.csv> [updates, default 6]"""
import csv
import sys

rows = []
for r in csv.DictReader(open(sys.argv[1])):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
last = int(sys.argv[2]) if len(sys.argv) > 2 else 6
marks = [i for i, (_, _, k) in enumerate(rows) if "k_env_step" in k]
runs = [(a, b) for a, b in zip(marks, marks[1:]) if b - a > 200]  # an update: between two runs of env steps
for a, b in runs[-last:]:
    first = next((i for i in range(a + 1, b) if "k_ppo_loss" in rows[i][2]), None)
    if first is None:
        continue
    seg = rows[a + 1:first]
    busy, cur = 0, rows[a][1]
    for s, e, _ in seg:
        if e > cur:
            busy += e - max(s, cur)
            cur = e
    span = rows[first][0] - rows[a][1]
    names = {}
    for _, _, k in seg:
        names[k[:40]] = names.get(k[:40], 0) + 1
    top = ", ".join(f"{n} {k}" for k, n in sorted(names.items(), key=lambda x: -x[1])[:5])
    print(f"update: rollout end -> first k_ppo_loss {span / 1e6:7.2f} ms, {len(seg)} dispatches, GPU busy "
          f"{busy / 1e6:6.2f} ms, idle {(span - busy) / 1e6:6.2f} ms; whole update {b - a - 1} dispatches; most: {top}")
