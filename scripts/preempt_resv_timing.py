"""Host wall time of the preemption dry run under Reservation
(KOORDHIP_PREEMPT_RESV) on the setup of DESIGN.md 4.12: 50k nodes, 24-36
assigned pods per node, with reservations added through synth.add_reservations
(tests/preempt_resv_model.py's generator: 70 % of the nodes hold one, with
--slots 4 up to four; about half of a node's listed pods are bound to one;
every other preemptor matches an owner group).

In one process, on the same table, alternating per call size:

  resv   koordhip_preempt_set_mode(RESV) under the profile with Reservation in
         the Filter: the walk starts from the restored row and keeps the
         plugin's AddPod / RemovePod state (k_preempt<NUMA, slots>)
  plain  the same profile without the Reservation plugin on the same table:
         the walk of the default mode (k_preempt<NUMA, 0>)

--numa puts NodeNUMAResource into both profiles (both legs set NUMA_FROZEN).
Each figure is the median of --reps timed calls after --warmup untimed ones;
every call synchronises.  Prints one JSON line.  Run it twice to see the spread.

--stream-sizes adds the sequential dry run, four legs
alternating per call size on the same two contexts:

  stream  koordhip_preempt_stream_resv: every preemptor on the state the
          earlier ones left, slots included
  batch   koordhip_preempt in the same mode: the independent batch
  loop    a host loop of n_pre one-preemptor koordhip_preempt calls
  chain   koordhip_preempt_stream with KOORDHIP_PREEMPT_STREAM_FULL=1 under the
          profile without the Reservation plugin: the per-preemptor chain
          without slots

and what the batch is worth for `batch` and `stream`: placed preemptors,
distinct nodes, victims claimed twice (of the first --max-victims per
preemptor).  A library without koordhip_preempt_stream_resv (KOORDHIP_LIB)
skips the `stream` leg.

    python scripts/preempt_resv_timing.py [--nodes 50000] [--base-per 24] [--slots 1] [--numa]
                                          [--reps 7] [--warmup 2] [--sizes 1,64,1024]
                                          [--stream-sizes 1,64,256,1024]
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


def worth(res, vic):
    """Placed preemptors, distinct nodes and victims more than one preemptor claims."""
    placed = res["node"][res["node"] >= 0]
    v = vic[vic >= 0]
    return {"placed": int(len(placed)), "nodes": int(len(set(placed.tolist()))),
            "claimed_twice": int(len(v) - len(set(v.tolist())))}


def stream_rows(er, ep, pres, ssizes, args):
    os.environ["KOORDHIP_PREEMPT_STREAM_FULL"] = "1"     # read at every koordhip_preempt_stream call
    mv = args.max_victims
    have = hasattr(er.lib, "koordhip_preempt_stream_resv")
    rows = []
    for k in ssizes:
        legs = [("batch", lambda: er.preempt(pres[:k], max_victims=mv)),
                ("loop", lambda: [er.preempt(pres[j:j + 1], max_victims=mv) for j in range(k)]),
                ("chain", lambda: ep.preempt_stream(pres[:k], max_victims=mv))]
        if have:
            legs.insert(0, ("stream", lambda: er.preempt_stream(pres[:k], max_victims=mv, resv=True)))
        times, out = {name: [] for name, _ in legs}, {}
        for r in range(args.warmup + args.reps):          # stream, batch, loop, chain, stream, ...
            for name, call in legs:
                t0 = time.perf_counter()
                out[name] = call()
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        row = {"n_pre": k}
        for name, _ in legs:
            row[name] = ms(times[name])
        for name in ("stream", "batch", "chain"):
            if name in out:
                row[name].update(worth(out[name][0], out[name][1]))
        if have:
            row["stream"]["stats"] = out["stream"][2]
            for name in ("batch", "loop", "chain"):
                row[f"stream_over_{name}"] = round(statistics.median(times["stream"]) / statistics.median(times[name]), 3)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--base-per", type=int, default=24)
    ap.add_argument("--slots", type=int, default=1)
    ap.add_argument("--numa", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,64,1024")
    ap.add_argument("--stream-sizes", default="")
    ap.add_argument("--max-victims", type=int, default=16)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    ssizes = [int(x) for x in args.stream_sizes.split(",") if x]
    import torch  # noqa: F401  (device discovery only)
    from koordinator_amd import abi
    from koordinator_amd.engine import PlacementEngine
    from koordinator_amd.snapshot import slot_col

    import preempt_model as M
    import preempt_resv_model as V

    inp = V.inputs(args.nodes, max(sizes + ssizes), M.SEED + 2, args.slots, False, args.numa, base_per=args.base_per)
    t, a, pres = inp.table, inp.assigned, inp.pres
    held = sum(((t[slot_col("resv_flags", q)] & abi.RESV_PRESENT) != 0).astype(int) for q in range(args.slots))
    o = {"nodes": args.nodes, "base_per": args.base_per, "slots": args.slots, "numa": args.numa, "reps": args.reps,
         "max_victims": args.max_victims, "assigned": int(len(a)),
         "bound": int(((a["flags"] & abi.ASG_RESV_SLOT_MASK) != 0).sum()),
         "nodes_with_reservations": int((held > 0).sum()), "reservations": int(held.sum()),
         "matching_preemptors": int((pres["pod"]["resv_match"] != 0).sum())}
    with PlacementEngine(inp.prof, device=0) as er, PlacementEngine(V.without_plugin(inp.prof), device=0) as ep:
        er.preempt_set_mode(numa_frozen=args.numa, resv=True)
        ep.preempt_set_mode(numa_frozen=args.numa)
        for e in (er, ep):
            e.load_snapshot(t)
            e.preempt_load_pods(a, inp.pdb_allowed)
        rows = []
        for k in sizes:
            tr, tp, out = [], [], {}
            for r in range(args.warmup + args.reps):      # resv, plain, resv, plain, ...
                for name, e, tt in (("resv", er, tr), ("plain", ep, tp)):
                    t0 = time.perf_counter()
                    out[name] = e.preempt(pres[:k], max_victims=args.max_victims)
                    if r >= args.warmup:
                        tt.append(time.perf_counter() - t0)
            row = {"n_pre": k, "resv": ms(tr), "plain": ms(tp),
                   "ratio": round(statistics.median(tr) / statistics.median(tp), 3)}
            for name in ("resv", "plain"):
                res = out[name][0]
                row[name]["placed"] = int((res["node"] >= 0).sum())
                row[name]["count"] = [int(x) for x in res["count"].sum(axis=0)]
            rows.append(row)
        o["rows"] = rows
        if ssizes:
            o["stream_rows"] = stream_rows(er, ep, pres, ssizes, args)
    print(json.dumps(o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
