"""Host wall time of a FitError's reasons on the setup of DESIGN.md 4.9: the
config-4 shape (50k nodes, Fit + LoadAware), a 20k-pod stream, the nodes' free
CPU tightened to --slack milli-CPU at most so that about a thousand pods stay
unplaced.  After one place call, in one process and alternating:

  (a) fetch_reasons(all pods)      lists + replay + 264 B per unplaced pod, decision states
  (b) fetch_diagnosis(all pods)    the same with 136-B per-plugin records: the yardstick
  (c) diagnose_reasons(unplaced)   final state, 264 B per pod
  (d) diagnose(unplaced)           final state, 136 B per pod: the yardstick
  (e) eval(unplaced, status)       the [pods][n] status plane to the host, the call alone (for scale)
  (f) fetch_node_reasons / fetch_node_status / node_reasons of one pod

Each figure is the median of --reps timed calls after --warmup untimed rounds;
every call synchronises.  Prints one JSON line.  Run it twice to see the spread.

    python scripts/reasons_timing.py [--nodes 50000] [--pods 20000] [--slack 4145] [--reps 7] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50000)
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--slack", type=int, default=4145)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch  # noqa: F401  (device discovery only)
    from koordinator_amd import abi, diagnosis, synth
    from koordinator_amd.config import shipped_profile
    from koordinator_amd.engine import PlacementEngine

    prof = shipped_profile()
    table, pods = synth.config_workload(4, prof, args.nodes, args.pods)
    free = (synth.uniform(synth.SEED, args.nodes, 901) * args.slack).astype(np.int64)
    table["requested0"][:] = np.maximum(table["requested0"], table["alloc0"] - free)
    pods["flags"][::3] |= abi.POD_DAEMONSET     # LoadAware lets them through: commits land on nodes it fails
    names = ("fetch_reasons", "fetch_diagnosis", "diagnose_reasons", "diagnose", "eval_status", "fetch_node_reasons",
             "fetch_node_status", "node_reasons")
    t = {k: [] for k in names}
    with PlacementEngine(prof, device=0) as eng:
        eng.load_snapshot(table)
        out = eng.place_stream(pods)
        un = np.flatnonzero(out < 0)
        if not len(un):
            print(json.dumps({"error": "no unplaced pod: lower --slack"}))
            return 1
        up, u0 = pods[un], int(un[len(un) // 2])
        for r in range(args.warmup + args.reps):
            calls = (("fetch_reasons", lambda: eng.fetch_reasons(len(pods))),
                     ("fetch_diagnosis", lambda: eng.fetch_diagnosis(len(pods))),
                     ("diagnose_reasons", lambda: eng.diagnose_reasons(up)),
                     ("diagnose", lambda: eng.diagnose(up)),
                     ("eval_status", lambda: eng.eval(up, status=True, scores=False)["status"]),
                     ("fetch_node_reasons", lambda: eng.fetch_node_reasons(u0)),
                     ("fetch_node_status", lambda: eng.fetch_node_status(u0)),
                     ("node_reasons", lambda: eng.node_reasons(pods[u0])))
            res = {}
            for name, call in calls:
                t0 = time.perf_counter()
                res[name] = call()
                if r >= args.warmup:
                    t[name].append(time.perf_counter() - t0)
        # the routes agree with each other: record against record, mask against status
        rs, dg = res["fetch_reasons"][un], res["fetch_diagnosis"][un]
        same = bool(np.array_equal(rs["feasible"], dg["feasible"]) and
                    np.array_equal(abi.reasons_status(res["fetch_node_reasons"]), res["fetch_node_status"]) and
                    np.array_equal(res["diagnose_reasons"]["feasible"], res["diagnose"]["feasible"]) and
                    np.array_equal(abi.reasons_status(res["node_reasons"]), res["eval_status"][len(un) // 2]))
        differ = int(sum(a != b for a, b in zip(rs, res["diagnose_reasons"])))
        helps = int(sum(diagnosis.preemption_might_help(x, args.nodes) for x in rs))
        example = diagnosis.fit_error_message(rs[0], args.nodes)
    o = {"nodes": args.nodes, "pods": args.pods, "slack_m": args.slack, "unplaced": int(len(un)),
         "decision_differs_from_final": differ, "preemption_might_help": helps, "reps": args.reps,
         "routes_agree": same, "example": example}
    for k, v in t.items():
        o[k + "_ms"] = round(statistics.median(v) * 1e3, 3)
        o[k + "_ms_min_max"] = [round(min(v) * 1e3, 3), round(max(v) * 1e3, 3)]
    print(json.dumps(o))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
