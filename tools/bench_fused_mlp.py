"""The fused value-guided greedy search against the stepped loop, scored by a FeatureMLP of the
reference's default widths (14 -> 256 -> 256 -> 128 -> 1, torch's default initialisation, seed 0),
feat_mean / feat_std = the tests' NORM_MEAN / NORM_STD, budget 10^4, not cyclical.

    python tools/bench_fused_mlp.py [--budget N] [--calls N] [--pops-per-launch N] [--out PATH]

Workload A: the 1,190 Miller-Schupp presentations (L = 18) in one call.  Workload B: AK(3) alone.
Each three ways, in one process on one device, each warmed by one full call and then timed
wall-clock (torch.cuda.synchronize() before and after) over --calls calls, every time listed:
  a  stepped, scorer = lambda x: model(x).squeeze(-1) with the torch module on the device: the path a
     caller had before acx.DeviceMLP;
  b  stepped, the acx.DeviceMLP of the same module as the scorer (acx_mlp_scores per step);
  c  fused (acx_vgreedy_run_mlp).
b and c score with one arithmetic, so their results must be equal (the tool fails otherwise); a's
scores are rocBLAS's, and the JSON says how many of its results equal c's.  Acceptance, per
workload: the median of c below the minimum of a.  Writes profiles/fused_mlp/bench_fused_mlp.json
and prints the same line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ac-solver-caltech_amd"))
import acx  # noqa: E402

NORM_MEAN = np.float32([12, 4, 5, 9, 2, 8, -5, 6, -2, 7, 3, -4, -1, 1])  # tests/beam_yardstick.py
NORM_STD = np.float32([-4, 2, -2, 8, -8, 16, -16, 32, -0.25, 0.125, 4, -32, 0.5, 1])
AK3 = [1, 1, 1, -2, -2, -2, -2, 1, 2, 1, -2, -1, -2]

ap = argparse.ArgumentParser()
ap.add_argument("--budget", type=int, default=10 ** 4)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--pops-per-launch", type=int, default=4096)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fused_mlp", "bench_fused_mlp.json"))
args = ap.parse_args()

DEV = torch.device("cuda:0")
nn = torch.nn
torch.manual_seed(0)
layers, prev = [], 14
for h in (256, 256, 128):
    layers += [nn.Linear(prev, h), nn.ReLU(), nn.Dropout(0.1)]
    prev = h
model = nn.Sequential(*layers, nn.Linear(prev, 1)).to(DEV).eval()
mlp = acx.DeviceMLP.from_module(model)

rows = acx.data.load_initial_states("all").astype(np.int32)
ak3 = np.zeros((1, 36), np.int32)
ak3[0, :7], ak3[0, 18:24] = AK3[:7], AK3[7:]


def call(pres, way):
    scorer = (lambda x: model(x).squeeze(-1)) if way == "a" else mlp
    return acx.value_guided_greedy_search_many(
        pres, scorer, args.budget, feat_mean=NORM_MEAN, feat_std=NORM_STD, device=DEV, on_error="return",
        return_stats=True, fused=(way == "c") if way != "a" else None, pops_per_launch=args.pops_per_launch)


def timed(pres, way):
    call(pres, way)  # warm-up: a full call
    times = []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call(pres, way)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return times, out


def same(x, y):
    return x[0] == y[0] and all(np.array_equal(x[1][k], y[1][k]) for k in x[1])


report = {"budget": args.budget, "calls": args.calls, "pops_per_launch": args.pops_per_launch,
          "widths": list(mlp.widths), "device": torch.cuda.get_device_name(DEV), "workloads": {}}
for name, pres in (("A", rows), ("B", ak3)):
    w = {"searches": len(pres)}
    outs = {}
    for way in "abc":
        times, outs[way] = timed(pres, way)
        w[way] = {"ms": [round(t, 3) for t in times], "median_ms": round(statistics.median(times), 3),
                  "min_ms": round(min(times), 3)}
    if not same(outs["b"], outs["c"]):
        raise SystemExit(f"workload {name}: the fused results differ from the stepped ones with the same scorer")
    st = outs["c"][1]
    w.update(pops_total=int(st["steps"].sum()), pops_max=int(st["steps"].max()), nodes_total=int(st["nodes"].sum()),
             launches_fused=-(-int(st["steps"].max()) // args.pops_per_launch),
             solved=int(sum(bool(r and r[0]) for r in outs["c"][0])),
             a_results_equal_c=int(sum(x == y for x, y in zip(outs["a"][0], outs["c"][0]))),
             c_median_below_a_min=w["c"]["median_ms"] < w["a"]["min_ms"])
    report["workloads"][name] = w
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(report, f, indent=1)
    f.write("\n")
print(json.dumps(report))
