"""Host wall time of the preemption dry run under DeviceShare beside Reservation
state (KOORDHIP_PREEMPT_DEVICE | KOORDHIP_PREEMPT_RESV |
KOORDHIP_PREEMPT_DEVICE_RESV) on the setup of DESIGN.md 4.10: 50k nodes, 24-36
assigned pods per node, with tests/preempt_resv_model.py's reservations (70 %
of the nodes hold one, with --slots 4 up to four; about half of a node's
listed pods are bound to one) and synth.add_devices' GPUs on every node, 20 %
of the listed pods holding a share of one; every fourth preemptor is a device
pod, every other one matches an owner group.

In one process, alternating per call size:

  both   the profile with DeviceShare and Reservation, all flags set: the walk
         that keeps both plugins' state (k_preempt_dev_resv<NUMA, slots, 2>)
  resv   the profile without DeviceShare on the same table without device
         columns, KOORDHIP_PREEMPT_RESV: k_preempt<NUMA, slots>
  dev    the profile without the Reservation plugin on the same cluster without
         reservation columns, KOORDHIP_PREEMPT_DEVICE: k_preempt_dev<NUMA, 2>

The three legs answer different questions (a device preemptor is a plain pod to
`resv`, a bound pod an ordinary one to `dev`), so every row carries the share
of CANDIDATE / UNFIT / UNRESOLVABLE pairs beside the time.  --numa puts
NodeNUMAResource into the three profiles (every leg sets NUMA_FROZEN).  Each
figure is the median of --reps timed calls after --warmup untimed ones; every
call synchronises.  Prints one JSON line.  Run it twice to see the spread.
--legs picks the legs (an A/B against a library without the combined mode,
KOORDHIP_LIB, runs resv,dev).

    python scripts/preempt_devresv_timing.py [--nodes 50000] [--base-per 24] [--slots 1] [--numa] [--reps 7]
                                             [--warmup 2] [--sizes 1,64,1024] [--dev-every 4] [--legs both,resv,dev]
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


def ms(v):
    return {"ms": round(statistics.median(v) * 1e3, 3), "min_max": [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--base-per", type=int, default=24)
    ap.add_argument("--slots", type=int, default=1)
    ap.add_argument("--numa", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--max-victims", type=int, default=16)
    ap.add_argument("--dev-pod-frac", type=float, default=0.2)
    ap.add_argument("--dev-every", type=int, default=4)
    ap.add_argument("--legs", default="both,resv,dev")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    names = [x for x in args.legs.split(",") if x]
    import torch  # noqa: F401  (device discovery only)
    from koordinator_amd import abi, synth
    from koordinator_amd.engine import PlacementEngine

    import preempt_dev_model as D
    import preempt_devresv_model as B
    import preempt_model as M
    import preempt_resv_model as V

    seed, n_pre = M.SEED + 2, max(sizes)
    spec = synth.DevSpec(gpu_frac=1.0, used_frac=0.3)
    o = {"nodes": args.nodes, "base_per": args.base_per, "slots": args.slots, "numa": args.numa, "reps": args.reps,
         "max_victims": args.max_victims, "lib": os.environ.get("KOORDHIP_LIB", "")}
    engines, legs = [], {}
    try:
        if "both" in names:
            inp, ext, ax = B.inputs(args.nodes, n_pre, seed, False, args.numa, args.slots, base_per=args.base_per,
                                    dev_every=args.dev_every, dev_spec=spec, dev_pod_frac=args.dev_pod_frac)
            e = PlacementEngine(inp.prof, device=0)
            engines.append(e)
            e.preempt_set_mode(numa_frozen=args.numa, resv=True, device=True, device_resv=True)
            e.load_snapshot(inp.table)
            e.preempt_load_pods(inp.assigned, inp.pdb_allowed, ext=ax)
            legs["both"] = (e, inp.pres, ext)
            bound = (inp.assigned["flags"] & abi.ASG_RESV_SLOT_MASK) != 0
            holds = (ax["dev_slots"] != 0).any(axis=1)
            o.update(assigned=int(len(inp.assigned)), bound=int(bound.sum()), device_pods=int(holds.sum()),
                     bound_device_pods=int((bound & holds).sum()),
                     device_preemptors=int(((ext["flags"] & abi.PODX_DEVICE) != 0).sum()),
                     matching_preemptors=int((inp.pres["pod"]["resv_match"] != 0).sum()))
        if "resv" in names:
            inp = V.inputs(args.nodes, n_pre, seed, args.slots, False, args.numa, base_per=args.base_per)
            e = PlacementEngine(inp.prof, device=0)
            engines.append(e)
            e.preempt_set_mode(numa_frozen=args.numa, resv=True)
            e.load_snapshot(inp.table)
            e.preempt_load_pods(inp.assigned, inp.pdb_allowed)
            legs["resv"] = (e, inp.pres, None)
        if "dev" in names:
            inp, ext, ax = D.inputs(args.nodes, n_pre, seed, False, args.numa, base_per=args.base_per,
                                    dev_pod_frac=args.dev_pod_frac, dev_every=args.dev_every, dev_spec=spec)
            e = PlacementEngine(inp.prof, device=0)
            engines.append(e)
            e.preempt_set_mode(numa_frozen=args.numa, device=True)
            e.load_snapshot(inp.table)
            e.preempt_load_pods(inp.assigned, inp.pdb_allowed, ext=ax)
            legs["dev"] = (e, inp.pres, ext)
        rows = []
        for k in sizes:
            times, out = {name: [] for name in legs}, {}
            for r in range(args.warmup + args.reps):      # both, resv, dev, both, ...
                for name, (e, pres, ext) in legs.items():
                    t0 = time.perf_counter()
                    out[name] = e.preempt(pres[:k], max_victims=args.max_victims, ext=None if ext is None else ext[:k])
                    if r >= args.warmup:
                        times[name].append(time.perf_counter() - t0)
            row = {"n_pre": k}
            for name in legs:
                res = out[name][0]
                cnt = res["count"].sum(axis=0).astype(float)
                row[name] = ms(times[name])
                row[name]["us_per_preemptor"] = round(statistics.median(times[name]) * 1e6 / k, 2)
                row[name]["placed"] = int((res["node"] >= 0).sum())
                row[name]["share"] = {s: round(float(cnt[c] / cnt.sum()), 4) for s, c in
                                      (("candidate", abi.PREEMPT_CANDIDATE), ("unfit", abi.PREEMPT_UNFIT),
                                       ("unresolvable", abi.PREEMPT_UNRESOLVABLE))}
            for name in ("resv", "dev"):
                if "both" in legs and name in legs:
                    row[f"both_over_{name}"] = round(statistics.median(times["both"]) / statistics.median(times[name]), 3)
            rows.append(row)
        o["rows"] = rows
    finally:
        for e in engines:
            e.close()
    print(json.dumps(o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
