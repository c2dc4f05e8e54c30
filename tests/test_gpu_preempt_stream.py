"""The sequential preemption dry run (koordhip_preempt_stream) on a real MI355X
against the oracle-only model (preempt_stream_model.py), bit for bit: results,
victims lists and the recompute counters; the A/B knob; the batch sizes; its
lack of side effects; the table / envelope errors."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, with_deviceshare

import preempt_model as M
import preempt_stream_model as S

pytestmark = pytest.mark.gpu

STAT_KEYS = ("full_recomputes", "block_recomputes", "blocks_skipped")


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, m):
    e = Engine(m.prof, device=0)
    e.load_snapshot(m.table)
    e.preempt_load_pods(m.assigned, m.pdb_allowed)
    return e


def assert_records_equal(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what} differs first at {bad}: got {got.reshape(-1)[bad]} want {want.reshape(-1)[bad]}")


def nblocks(m):
    return (m.table.n + S.BLOCK - 1) // S.BLOCK


# ------------------------------------------------------ 1. results and victims
@pytest.mark.parametrize("name", S.CASES)
def test_stream_results_and_victims(Engine, name):
    """The six cases of the independent dry run, `clean`, `prio` and the
    directed cases (the second overlay word, a chain of nominated pods, a spent
    budget, a floored quota, three phase-1 tiles); victims at
    max_victims 0, exact and truncated.  The later calls run in the same
    context: the call's own state is set up anew every time."""
    m = S.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(m.pres, max_victims=exact)
        res0, vic0, st0 = e.preempt_stream(m.pres, max_victims=0)
        res1, vic1, st1 = e.preempt_stream(m.pres, max_victims=1)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert_records_equal(res0, m.res, f"{name}: results without victims")
    assert vic0.shape == (len(m.pres), 0)
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    assert (res["count"].sum(axis=1) == m.table.n).all()
    # which blocks the engine evaluates again follows from the results alone: the model keeps the same books
    for s in (st, st0, st1):
        assert {k: s[k] for k in STAT_KEYS} == {k: m.stats[k] for k in STAT_KEYS}, name
    assert st["block_recomputes"] + st["blocks_skipped"] == len(m.pres) * nblocks(m)


def test_truncation_is_exercised():
    assert any(int(S.case(c).res["best"]["n_victims"].max()) > 1 for c in S.CASES)


# ------------------------------------------------------------ 2. A/B and stats
@pytest.mark.parametrize("name", ["tiles", "clean", "prio", "la257"] + list(S.DIRECTED))
def test_full_recompute_gives_the_same_answers(Engine, name, monkeypatch):
    """KOORDHIP_PREEMPT_STREAM_FULL is read at every call, so both runs share
    this process; each gets a fresh context."""
    m = S.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    monkeypatch.delenv("KOORDHIP_PREEMPT_STREAM_FULL", raising=False)
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(m.pres, max_victims=exact)
    monkeypatch.setenv("KOORDHIP_PREEMPT_STREAM_FULL", "1")
    with loaded(Engine, m) as e:
        resf, vicf, stf = e.preempt_stream(m.pres, max_victims=exact)
    assert_records_equal(resf, res, f"{name}: results, every block recomputed")
    assert_records_equal(vicf, vic, f"{name}: victims, every block recomputed")
    assert_records_equal(resf, m.res, f"{name}: results against the model")
    assert stf["block_recomputes"] == len(m.pres) * nblocks(m) and stf["blocks_skipped"] == 0
    assert st["block_recomputes"] < stf["block_recomputes"]


def test_stats_of_clean_and_tiles(Engine):
    with loaded(Engine, S.case("clean")) as e:
        _, _, st = e.preempt_stream(S.case("clean").pres)
    assert st["full_recomputes"] == 0 and st["blocks_skipped"] > 0
    with loaded(Engine, S.case("tiles")) as e:
        _, _, st = e.preempt_stream(S.case("tiles").pres)
    assert st["full_recomputes"] > 0


# ------------------------------------------------------------- 3. batch sizes
def test_batch_sizes(Engine):
    m, ind = S.case("tiles"), M.case("tiles")
    assert len(m.pres) == 33
    with loaded(Engine, m) as e:
        res0, vic0, st0 = e.preempt_stream(m.pres[:0], max_victims=2)
        res1, vic1, _ = e.preempt_stream(m.pres[:1], max_victims=4)
        one, onev = e.preempt(m.pres[:1], max_victims=4)
        res7, vic7, _ = e.preempt_stream(m.pres[:7], max_victims=4)
        res33, _, _ = e.preempt_stream(m.pres)
    assert res0.shape == (0,) and vic0.shape == (0, 2) and st0 == dict.fromkeys(STAT_KEYS, 0)
    assert_records_equal(res1, one, "one preemptor: the independent dry run's result")
    assert_records_equal(vic1, onev, "one preemptor: the independent dry run's victims")
    assert_records_equal(res1, ind.res[:1], "one preemptor against the model")
    assert_records_equal(res7, m.res[:7], "a prefix of the batch is the batch's prefix")
    assert_records_equal(vic7, M.victims_array(m.chosen[:7], 4), "a prefix's victims")
    assert_records_equal(res33, m.res, "33 preemptors")


# ------------------------------------------------------- 4. no side effects
def test_stream_changes_no_state(Engine):
    m, ind = S.case("tiles"), M.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, seed=11), m.prof)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        plain = e.place_stream(stream)
    with loaded(Engine, m) as e:
        n0 = e.read_nodes()
        before, vbefore = e.preempt(m.pres, max_victims=4)
        e.preempt_stream(m.pres, max_victims=4)
        n1 = e.read_nodes()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        after, vafter = e.preempt(m.pres, max_victims=4)     # the loaded table and budgets are as they were
        ver = e.preempt_node_verdicts(m.pres[5])
        placed = e.place_stream(stream)
    assert_records_equal(after, before, "koordhip_preempt after the stream")
    assert_records_equal(vafter, vbefore, "koordhip_preempt's victims after the stream")
    assert_records_equal(after, ind.res, "koordhip_preempt against its model")
    assert_records_equal(ver, ind.verdicts[5], "verdicts after the stream")
    assert np.array_equal(placed, plain)
    assert np.array_equal(plain, oracle.Oracle(m.cfg, m.table).place_stream(stream))


# ------------------------------------------------------------------ 5. errors
def expect(code, call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == code, ei.value


def test_estate_without_a_table(Engine):
    m = S.case("wave")
    with Engine(m.prof, device=0) as e:
        expect(abi.E_STATE, lambda: e.preempt_stream(m.pres))          # no snapshot
        e.load_snapshot(m.table)
        expect(abi.E_STATE, lambda: e.preempt_stream(m.pres))          # no table
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        e.preempt_stream(m.pres)
        e.load_snapshot(m.table)                                       # invalidates the table
        expect(abi.E_STATE, lambda: e.preempt_stream(m.pres))


def test_reserve_pod_as_preemptor_is_einval(Engine):
    m = S.case("wave")
    pre = m.pres.copy()
    pre["pod"]["flags"][1] |= abi.POD_RESERVE
    bad_quota = m.pres.copy()
    bad_quota["quota"][0] = -2
    bad_mask = m.pres.copy()
    bad_mask["q_mask"][2] = 1 << abi.PREEMPT_QRES
    with loaded(Engine, m) as e:
        expect(abi.E_INVAL, lambda: e.preempt_stream(pre))
        expect(abi.E_INVAL, lambda: e.preempt_stream(bad_quota))
        expect(abi.E_INVAL, lambda: e.preempt_stream(bad_mask))
        res, _, _ = e.preempt_stream(m.pres)                           # a refused call leaves the context usable
    assert_records_equal(res, m.res, "results after refused calls")


@pytest.mark.parametrize("kind", ["numa", "reservation", "sequential"])
def test_envelope_is_einval(Engine, kind):
    prof = {"numa": lambda: shipped_profile(numa=True), "reservation": lambda: shipped_profile(reservation=True),
            "sequential": lambda: with_deviceshare(shipped_profile())}[kind]()
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    if kind == "numa":
        synth.add_numa(table, synth.NumaSpec(), prof)
    if kind == "reservation":
        synth.add_reservations(table, synth.ResvSpec())
    if kind == "sequential":
        synth.add_devices(table, synth.DevSpec())
    m = M.case("wave")
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)     # 63 nodes' pods fit 64 nodes: the table itself is fine
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres))
