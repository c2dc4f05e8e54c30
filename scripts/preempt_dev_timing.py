"""Host wall time of the preemption dry run under DeviceShare
(KOORDHIP_PREEMPT_DEVICE) on the setup of DESIGN.md 4.10: 50k nodes, 24-36
assigned pods per node, with devices added by tests/preempt_dev_model.py's
generator: GPUs on every node (synth.add_devices with gpu_frac 1), 20 % of
the listed pods holding a share of one, 1024 preemptors.

In one process, on the same rows, alternating per call size:

  dev2   the DeviceShare profile with the flag set, every fourth preemptor a
         device pod: the walk that moves scalars and devices (k_preempt_dev<NUMA, 2>)
  dev1   the same context, the same preemptors without any device or scalar
         request: the scalars-only walk (k_preempt_dev<NUMA, 1>)
  plain  the profile without DeviceShare on the same rows without device
         columns: the walk of the default mode (k_preempt<NUMA, 0>)

--stream times the sequential dry run of the mode instead, on the dev2 batch
and the same context, alternating per call size:

  stream  koordhip_preempt_stream_ext: every preemptor on the state the
          earlier ones left (k_preempt_seq_dev / k_preempt_apply_dev)
  batch   koordhip_preempt_ext: the independent batch
  loop    a host loop of one-preemptor koordhip_preempt_ext calls, what a host
          could do before the call existed (the table stays stale: its answers
          are the batch's)

and reports the stream's stats, over how many nodes the placed preemptors
spread and how many victims more than one preemptor claims.

Each figure is the median of --reps timed calls after --warmup untimed ones;
every call synchronises.  Prints one JSON line.  Run it twice to see the spread.

    python scripts/preempt_dev_timing.py [--nodes 50000] [--base-per 24] [--reps 7] [--warmup 2]
                                         [--sizes 1,64,1024] [--dev-pod-frac 0.2] [--dev-every 4] [--stream]
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


def claimed_twice(vic):
    """Victims more than one preemptor of the batch claims (vic [p][max_victims], -1 padded)."""
    import numpy as np
    v = vic[vic >= 0]
    _, c = np.unique(v, return_counts=True)
    return int((c > 1).sum())


def stream_rows(e, pres, ext, sizes, args):
    rows = []
    mv = args.max_victims

    def loop(k):
        out = [e.preempt(pres[p:p + 1], max_victims=mv, ext=ext[p:p + 1]) for p in range(k)]
        return out[-1]

    for k in sizes:
        legs = (("stream", lambda: e.preempt_stream(pres[:k], max_victims=mv, ext=ext[:k])),
                ("batch", lambda: e.preempt(pres[:k], max_victims=mv, ext=ext[:k])),
                ("loop", lambda: loop(k)))
        times, out = {name: [] for name, _ in legs}, {}
        for r in range(args.warmup + args.reps):      # stream, batch, loop, stream, ...
            for name, call in legs:
                t0 = time.perf_counter()
                out[name] = call()
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        row = {"n_pre": k}
        for name, _ in legs:
            row[name] = ms(times[name])
            row[name]["us_per_preemptor"] = round(statistics.median(times[name]) * 1e6 / k, 2)
        for name in ("stream", "batch"):
            res, vic = out[name][0], out[name][1]
            placed = res["node"][res["node"] >= 0]
            row[name].update(placed=int(len(placed)), nodes=int(len(set(placed.tolist()))),
                             victims=int((vic >= 0).sum()), claimed_twice=claimed_twice(vic))
        row["stream"]["stats"] = out["stream"][2]
        row["stream_over_batch"] = round(statistics.median(times["stream"]) / statistics.median(times["batch"]), 3)
        row["stream_over_loop"] = round(statistics.median(times["stream"]) / statistics.median(times["loop"]), 3)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--base-per", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--max-victims", type=int, default=16)
    ap.add_argument("--dev-pod-frac", type=float, default=0.2)
    ap.add_argument("--dev-every", type=int, default=4)
    ap.add_argument("--stream", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    import torch  # noqa: F401  (device discovery only)
    from koordinator_amd import abi, synth
    from koordinator_amd.engine import PlacementEngine

    import preempt_dev_model as D
    import preempt_model as M

    seed = M.SEED + 2
    plain = M.inputs("base", args.nodes, max(sizes), seed, False, args.base_per)
    inp, ext, ax = D.inputs(args.nodes, max(sizes), seed, False, False, base_per=args.base_per,
                            dev_pod_frac=args.dev_pod_frac, dev_every=args.dev_every,
                            dev_spec=synth.DevSpec(gpu_frac=1.0, used_frac=0.3))
    t, a, pres = inp.table, inp.assigned, inp.pres
    none = abi.pod_ext_array(len(pres))
    o = {"nodes": args.nodes, "base_per": args.base_per, "reps": args.reps, "max_victims": args.max_victims,
         "assigned": int(len(a)), "device_pods": int((ax["dev_slots"] != 0).any(axis=1).sum()),
         "scalar_pods": int((ax["xmask"] != 0).sum()),
         "device_preemptors": int(((ext["flags"] & abi.PODX_DEVICE) != 0).sum()),
         "lib": os.environ.get("KOORDHIP_LIB", "")}
    if args.stream:
        with PlacementEngine(inp.prof, device=0) as ed:
            ed.preempt_set_mode(device=True)
            ed.load_snapshot(t)
            ed.preempt_load_pods(a, inp.pdb_allowed, ext=ax)
            o["stream_rows"] = stream_rows(ed, pres, ext, sizes, args)
        print(json.dumps(o))
        return 0
    with PlacementEngine(inp.prof, device=0) as ed, PlacementEngine(plain.prof, device=0) as ep:
        ed.preempt_set_mode(device=True)
        ed.load_snapshot(t)
        ed.preempt_load_pods(a, inp.pdb_allowed, ext=ax)
        ep.load_snapshot(plain.table)
        ep.preempt_load_pods(plain.assigned, plain.pdb_allowed)
        rows = []
        for k in sizes:
            legs = (("dev2", ed, ext[:k]), ("dev1", ed, none[:k]), ("plain", ep, None))
            times, out = {name: [] for name, _, _ in legs}, {}
            for r in range(args.warmup + args.reps):      # dev2, dev1, plain, dev2, ...
                for name, e, x in legs:
                    t0 = time.perf_counter()
                    out[name] = e.preempt(pres[:k], max_victims=args.max_victims, ext=x)
                    if r >= args.warmup:
                        times[name].append(time.perf_counter() - t0)
            row = {"n_pre": k}
            for name, _, _ in legs:
                res = out[name][0]
                row[name] = ms(times[name])
                row[name]["us_per_preemptor"] = round(statistics.median(times[name]) * 1e6 / k, 2)
                row[name]["placed"] = int((res["node"] >= 0).sum())
                row[name]["count"] = [int(x) for x in res["count"].sum(axis=0)]
            for name in ("dev2", "dev1"):
                row[name + "_ratio"] = round(statistics.median(times[name]) / statistics.median(times["plain"]), 3)
            rows.append(row)
        o["rows"] = rows
    print(json.dumps(o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
