"""Host wall time of the preemption dry run under NodeNUMAResource on the setup
of DESIGN.md 4.10: 50k nodes, 24-36 assigned pods per node (the generator of
tests/preempt_numa_model.py with base_per=24), config 3's NUMA columns plus
amplified and topology-policy nodes, half the preemptors cpuset pods.

In one process, on the same table, alternating per call size:

  numa   koordhip_preempt_set_mode(NUMA_FROZEN) under the profile with
         NodeNUMAResource in the Filter: k_preempt_numa's plane, then the walk
         reading it and evaluating filterAmplifiedCPUs on every row
  plain  the Fit + LoadAware profile: the same walk without the plane and
         without filterAmplifiedCPUs

for koordhip_preempt (--sizes) and koordhip_preempt_stream (--stream-sizes).
Each figure is the median of --reps timed calls after --warmup untimed ones;
every call synchronises.  Prints one JSON line.  Run it twice to see the spread.

--default-mode times koordhip_preempt alone, in the default mode, on
tests/preempt_model.py's generator (no NUMA columns): the path that must not
move.  It calls nothing a build before this feature lacks, so KOORDHIP_LIB can
name such a build for an A/B on one device.

    python scripts/preempt_numa_timing.py [--nodes 50000] [--base-per 24] [--reps 7] [--warmup 2]
                                          [--sizes 1,64,1024] [--stream-sizes 64,256] [--default-mode]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, reps, warmup):
    t, out = [], None
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        if r >= warmup:
            t.append(time.perf_counter() - t0)
    return t, out


def ms(v):
    return {"ms": round(statistics.median(v) * 1e3, 3), "min_max": [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--base-per", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--stream-sizes", default="64,256")
    ap.add_argument("--max-victims", type=int, default=16)
    ap.add_argument("--default-mode", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    ssizes = [int(x) for x in args.stream_sizes.split(",") if x]
    n_pre = max(sizes + ssizes)
    import torch  # noqa: F401  (device discovery only)
    from koordinator_amd import abi, synth
    from koordinator_amd.config import shipped_profile
    from koordinator_amd.engine import PlacementEngine

    import preempt_model as M
    import preempt_numa_model as N

    o = {"nodes": args.nodes, "base_per": args.base_per, "reps": args.reps, "max_victims": args.max_victims,
         "lib": os.environ.get("KOORDHIP_LIB", "")}
    if args.default_mode:
        inp = M.inputs("base", args.nodes, n_pre, M.SEED + 2, False, args.base_per)
        o["assigned"] = int(len(inp.assigned))
        with PlacementEngine(inp.prof, device=0) as e:
            e.load_snapshot(inp.table)
            e.preempt_load_pods(inp.assigned, inp.pdb_allowed)
            for k in sizes:
                t, (res, _) = timed(lambda: e.preempt(inp.pres[:k], max_victims=args.max_victims), args.reps, args.warmup)
                o[f"preempt_{k}"] = dict(ms(t), placed=int((res["node"] >= 0).sum()))
        print(json.dumps(o))
        return 0

    spec = synth.NumaSpec(amp_frac=0.2, policy_frac=0.2)       # config 3's columns + amplified + policy nodes
    inp = N.inputs(args.nodes, n_pre, M.SEED + 2, spec, False, base_per=args.base_per, cpuset_of=2)
    pres = inp.pres
    o["assigned"] = int(len(inp.assigned))
    o["cpuset_preemptors"] = int(((pres["pod"]["flags"] & abi.POD_CPUSET) != 0).sum())
    o["amplified_nodes"] = int((inp.table["numa_amp_cpu"] > 1.0).sum())
    o["policy_nodes"] = int((((inp.table["numa_flags"] >> abi.NODE_NUMA_POLICY_SHIFT) & 3) != 0).sum())
    with PlacementEngine(inp.prof, device=0) as en, PlacementEngine(shipped_profile(), device=0) as ep:
        en.preempt_set_mode(numa_frozen=True)
        for e in (en, ep):
            e.load_snapshot(inp.table)
            e.preempt_load_pods(inp.assigned, inp.pdb_allowed)
        rows = []
        for kind, ks in (("preempt", sizes), ("preempt_stream", ssizes)):
            for k in ks:
                tn, tp, out = [], [], {}
                for r in range(args.warmup + args.reps):      # numa, plain, numa, plain, ...
                    for name, e, t in (("numa", en, tn), ("plain", ep, tp)):
                        t0 = time.perf_counter()
                        out[name] = getattr(e, kind)(pres[:k], max_victims=args.max_victims)
                        if r >= args.warmup:
                            t.append(time.perf_counter() - t0)
                row = {"call": kind, "n_pre": k, "numa": ms(tn), "plain": ms(tp),
                       "ratio": round(statistics.median(tn) / statistics.median(tp), 3)}
                for name in ("numa", "plain"):
                    res = out[name][0]
                    row[name]["placed"] = int((res["node"] >= 0).sum())
                    row[name]["count"] = [int(x) for x in res["count"].sum(axis=0)]
                rows.append(row)
        o["rows"] = rows
    print(json.dumps(o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
