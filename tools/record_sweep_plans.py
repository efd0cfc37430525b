#!/usr/bin/env python3
"""Developer tool: record tests/golden/sweep_plans.json - the plan in force after every step of the sequences of
tests/sweep_plan_sequences.py, on the device at hand (tests/test_gpu_sweep_plan_golden.py replays them, tests/test_sweep_plan_cpu.py
holds the device-free planner to the recorded plans).  Run it on the commit whose plans are the specification.

  python tools/record_sweep_plans.py [output file]

Equal plans are stored once: {"plans": [{tiles, info, weight}], "sequences": [{name, shape, env, steps: [index into plans]}]}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import sweep_plan_sequences as sq  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "sweep_plans.json")
plans, index, seqs, fields = [], {}, [], {}
for seq in sq.sequences():
    name, shape, env, steps = seq
    if shape not in fields:
        fields[shape] = torch.from_numpy(sq.field_of(shape)).cuda()
    at = []
    for p in sq.replay(seq, fields[shape]):
        key = json.dumps(p, sort_keys=True)
        if key not in index:
            index[key] = len(plans)
            plans.append(p)
        at.append(index[key])
    seqs.append({"name": name, "shape": shape, "env": env, "steps": at})
    print("%-28s %s" % (name, " ".join("%d:%d%s" % (k, plans[k]["info"][0], "t" if plans[k]["info"][2] else "") for k in at)))
with open(out, "w") as f:
    json.dump({"plans": plans, "sequences": seqs}, f, separators=(",", ":"))
    f.write("\n")
print("%d plans of %d steps, resident blocks %s, %d bytes" % (len(plans), sum(len(s["steps"]) for s in seqs),
                                                             sorted({p["info"][1] for p in plans}), os.path.getsize(out)))
