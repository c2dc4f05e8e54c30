"""The hand-worked cases of the preemption dry run (preempt_cases.py) on a real
MI355X, compared with the hand-written literals first and with the model
(preempt_model.py) second, so that an error the model and the kernels share
still fails.

1. Every case of the per-node walk, one or two nodes each, through
   koordhip_preempt_node_verdicts, koordhip_preempt with max_victims = the
   exact count, and koordhip_preempt_stream with the single preemptor.
2. The pick, in one cluster of 16641 nodes (66 workgroups of 256, the last
   with one live lane) that holds 116 independent contests: two (once three)
   candidate nodes per preemptor, every other node NO_VICTIMS for it.  One call
   answers all of them: grid.y = 4 tiles of 32 preemptors, the last ragged.
   Every contest's expected answer is its two-node case's literal, put at the
   contest's nodes; test_preempt_model.py checks that construction on the CPU
   (each contest is decided at the level it is named for and at no earlier one).
3. The same batch through koordhip_preempt_stream, with and without
   KOORDHIP_PREEMPT_STREAM_FULL: the contests share no node, no quota and no
   budget above 0, so the answers are koordhip_preempt's.

What pins what.  A contest is named level/placement/orientation; "lo" has the
better node at the lower index, "hi" at the higher.  Flipping the comparison
of one branch of pick_before, or losing a field on the way through one stage,
changes the winner of the contests of that row and column:

  branch of pick_before            contests (every placement, lo and hi)
  na < 0 / nb < 0 (no candidate)   all: 254 of a workgroup's 256 lanes, 64 of
                                   the pick's 66 partials hold none
  za != zb   (no victims wins)     zero/*
  n_pdb_violations                 pdb/*
  top_priority                     top/*, top_lowest/*, top_highest/* (signed:
                                   -2^31 against -2^31 + 1)
  sum_priority                     sum/*, sum_high_half/*, sum_low_half/*,
                                   sum_halves_disagree/*
  n_victims                        count/* (needs a victim of priority -2^31)
  earliest_start (latest wins)     start/*, start_high_half/*, start_low_half/*,
                                   start_halves_disagree/*, start_sign/*,
                                   start_min_max/*, start_min/*
  na < nb                          index/* (lo and hi: the lower index wins
                                   both times), three

  stage of the reduction           placement
  wave shuffle (wave_best)         */wave/*: lanes t and 63 - t of one wave, so
                                   every shuffle offset carries a winner, in
                                   both directions; all 64 bits of sum and
                                   start by the half and sign contests
  workgroup LDS (block_best)       */lanes/*: lanes 63 | 64, adjacent waves
  partials, strided loop           */strided/*: workgroups b and b + 64 meet in
                                   one lane on the loop's second trip
  partials, 64-lane shuffle        (k_preempt_pick's wave_best)
                                   */groups/* (nodes 255 | 256, adjacent
                                   lanes), */far/* (workgroups 1 and 33: shuffle
                                   offset 32 alone), start/ragged/hi
                                   (workgroups 0 and 65: the winner is the one
                                   live lane of the last workgroup, met on the
                                   loop's second trip), three (three
                                   workgroups); the half and sign contests run
                                   at far as well
  koordhip_preempt_stream          the same contests through k_preempt_blk,
                                   k_preempt_seq (the touched workgroups) and
                                   k_preempt_seq_pick's loop and wave_best
"""
import numpy as np
import pytest

from koordinator_amd.config import to_c_config

import preempt_cases as K
import preempt_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, prof, table, assigned, pdb):
    e = Engine(prof, device=0)
    e.load_snapshot(table)
    e.preempt_load_pods(assigned, pdb)
    return e


def assert_records_equal(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what} differs first at {bad}: got {got.reshape(-1)[bad]} want {want.reshape(-1)[bad]}")


# ------------------------------------------------------------- 1. the walk
@pytest.mark.parametrize("name", list(K.WALK))
def test_walk_case(Engine, name):
    c = K.WALK[name]
    a, t = c.assigned, c.table
    exact = max(1, len(c.vic[c.node])) if c.node >= 0 else 1
    with loaded(Engine, c.prof, t, a, c.pdb) as e:
        ver = e.preempt_node_verdicts(c.pre)
        res, vic = e.preempt(c.pre, max_victims=exact)
        sres, svic, _ = e.preempt_stream(c.pre, max_victims=exact)
    # the literals
    assert [tuple(int(x) for x in v) for v in ver] == c.ver
    assert int(res["node"][0]) == c.node and list(res["count"][0]) == c.count
    assert tuple(res["best"][0].item()) == c.best
    assert_records_equal(ver, K.verdict_records(c.ver), f"{name}: verdicts")
    assert_records_equal(res[0], K.result_record(c.node, c.count, c.best), f"{name}: result")
    chosen = [c.vic[c.node] if c.node >= 0 else []]
    assert_records_equal(vic, M.victims_array(chosen, exact), f"{name}: victims")
    if c.lists is not None:
        assert vic[0].tolist() == c.lists[c.node]
    # a batch of one is the independent dry run
    assert_records_equal(sres, res, f"{name}: the stream's result")
    assert_records_equal(svic, vic, f"{name}: the stream's victims")
    # the model
    mver, mvic, _ = M.select_victims(to_c_config(c.prof), t, a, c.pdb, c.pre)
    assert_records_equal(ver, mver, f"{name}: verdicts against the model")
    assert_records_equal(res[0], M.pick(mver), f"{name}: result against the model")
    assert mvic == c.vic


# ------------------------------------------------------------- 2. the pick
@pytest.fixture(scope="module")
def cluster():
    return K.contest_cluster()


@pytest.fixture(scope="module")
def answers(Engine, cluster):
    """One snapshot load, one table load and three calls; the A/B knob is read at every call."""
    import os
    cl = cluster
    old = os.environ.pop("KOORDHIP_PREEMPT_STREAM_FULL", None)
    try:
        with loaded(Engine, cl.prof, cl.table, cl.assigned, cl.pdb_allowed) as e:
            ind = e.preempt(cl.pres, max_victims=cl.max_victims)
            seq = e.preempt_stream(cl.pres, max_victims=cl.max_victims)
            os.environ["KOORDHIP_PREEMPT_STREAM_FULL"] = "1"
            full = e.preempt_stream(cl.pres, max_victims=cl.max_victims)
    finally:
        os.environ.pop("KOORDHIP_PREEMPT_STREAM_FULL", None)
        if old is not None:
            os.environ["KOORDHIP_PREEMPT_STREAM_FULL"] = old
    return ind, seq, full


def assert_contests(cluster, res, vic, what):
    wrong = []
    for ct in cluster.contests:
        r = res[ct.quota]
        got = (int(r["node"]), tuple(r["best"].item()), list(r["count"]), [int(x) for x in vic[ct.quota] if x >= 0])
        want = (ct.node, tuple(ct.best), ct.count, ct.victims)
        if got != want:
            wrong.append(f"{ct.name} at nodes {ct.nodes}: got {got} want {want}")
    assert not wrong, f"{what}: {len(wrong)} of {len(cluster.contests)} contests\n" + "\n".join(wrong)
    assert_records_equal(res, cluster.res, what)
    assert_records_equal(vic, cluster.victims, f"{what}: victims")


def test_contest_cluster_pick(cluster, answers):
    res, vic = answers[0]
    assert_contests(cluster, res, vic, "koordhip_preempt")
    assert (res["count"].sum(axis=1) == K.CLUSTER_N).all()


def test_contest_cluster_stream(cluster, answers):
    (res, vic), (sres, svic, st), (fres, fvic, fst) = answers
    assert_contests(cluster, sres, svic, "koordhip_preempt_stream")
    assert_records_equal(sres, res, "the stream's results against koordhip_preempt's")
    assert_records_equal(svic, vic, "the stream's victims against koordhip_preempt's")
    total = len(cluster.pres) * K.CLUSTER_BLOCKS
    assert st["block_recomputes"] + st["blocks_skipped"] == total
    assert st["full_recomputes"] == 0 and st["blocks_skipped"] > 0
    assert_contests(cluster, fres, fvic, "koordhip_preempt_stream, every block recomputed")
    assert fst["block_recomputes"] == total and fst["blocks_skipped"] == 0
