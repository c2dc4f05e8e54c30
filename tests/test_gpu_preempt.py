"""The preemption dry run on a real MI355X against the oracle-only model
(preempt_model.py), bit for bit: koordhip_preempt_node_verdicts (every node's
verdict), koordhip_preempt (results and victims lists), its lack of side
effects, and the table / envelope errors."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, with_deviceshare

import preempt_model as M

pytestmark = pytest.mark.gpu


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


# ------------------------------------------------------- 1. per-node verdicts
@pytest.mark.parametrize("name", list(M.CASES))
def test_node_verdicts(Engine, name):
    """One lane, a partial wave, a ragged second tile; a node holding 128 pods; static filters."""
    m = M.case(name)
    picks = sorted({0, len(m.pres) // 2, len(m.pres) - 1} | set(range(min(len(m.pres), 4))))
    with loaded(Engine, m) as e:
        got = {p: e.preempt_node_verdicts(m.pres[p]) for p in picks}
    for p in picks:
        assert_records_equal(got[p], m.verdicts[p], f"{name}: verdicts of preemptor {p}")


# ------------------------------------------------------ 2. results and victims
@pytest.mark.parametrize("name", list(M.CASES))
def test_preempt_results_and_victims(Engine, name):
    m = M.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic = e.preempt(m.pres, max_victims=exact)
        res0, vic0 = e.preempt(m.pres, max_victims=0)
        res1, vic1 = e.preempt(m.pres, max_victims=1)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert_records_equal(res0, m.res, f"{name}: results without victims")
    assert vic0.shape == (len(m.pres), 0)
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")   # best.n_victims tells the full count
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    assert (res["count"].sum(axis=1) == m.table.n).all()


def test_truncation_is_exercised():
    assert any(int(M.case(c).res["best"]["n_victims"].max()) > 1 for c in M.CASES)


def test_full_node_holds_128():
    m = M.case("full")
    assert int((m.assigned["node"] == M.FULL_NODE).sum()) == abi.PREEMPT_NODE_PODS
    assert any(len(m.potential[p][M.FULL_NODE]) > 0 and m.verdicts[p]["status"][M.FULL_NODE] == abi.PREEMPT_CANDIDATE
               for p in range(len(m.pres)))


# ------------------------------------------------------- 3. no side effects
def test_preempt_changes_no_state(Engine):
    m = M.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, seed=11), m.prof)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        plain = e.place_stream(stream)
    with loaded(Engine, m) as e:
        n0 = e.read_nodes()
        e.preempt(m.pres, max_victims=4)
        e.preempt_node_verdicts(m.pres[0])
        n1 = e.read_nodes()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        after = e.place_stream(stream)
        res, _ = e.preempt(m.pres[:1])          # the table outlives a place call; the state it ran on has moved
    assert np.array_equal(after, plain)
    assert np.array_equal(plain, oracle.Oracle(m.cfg, m.table).place_stream(stream))
    assert res["count"].sum() == m.table.n


def test_reload_replaces_the_table(Engine):
    """A second preempt_load_pods replaces the first; an empty table leaves no victims anywhere."""
    m = M.case("wave")
    with loaded(Engine, m) as e:
        e.preempt_load_pods(m.assigned[:0], ())
        res, _ = e.preempt(m.pres)
        assert (res["node"] == -1).all()
        assert (res["count"][:, abi.PREEMPT_NO_VICTIMS] == m.table.n).all()
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        res, _ = e.preempt(m.pres)
    assert_records_equal(res, m.res, "results after the reload")


# ------------------------------------------------------------------ 4. errors
def expect(code, call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == code, ei.value


def test_load_pods_errors(Engine):
    m = M.case("wave")
    with Engine(m.prof, device=0) as e:
        expect(abi.E_STATE, lambda: e.preempt_load_pods(m.assigned, m.pdb_allowed))   # no snapshot
        e.load_snapshot(m.table)
        expect(abi.E_STATE, lambda: e.preempt(m.pres))                               # no table
        expect(abi.E_STATE, lambda: e.preempt_node_verdicts(m.pres[0]))
        a = np.zeros(abi.PREEMPT_NODE_PODS + 1, abi.ASSIGNED_DTYPE)
        a["node"] = 7
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(a, ()))                       # 129 pods on a node
        e.preempt_load_pods(a[:abi.PREEMPT_NODE_PODS], ())
        for node in (-1, m.table.n):
            b = m.assigned[:3].copy()
            b["node"][1] = node
            expect(abi.E_INVAL, lambda: e.preempt_load_pods(b, m.pdb_allowed))        # node out of range
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(m.assigned, (1,) * (abi.PREEMPT_PDBS + 1)))  # 9 PDBs
        b = m.assigned[:3].copy()
        b["pdb_mask"][2] = 1 << M.N_PDB
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(b, m.pdb_allowed))            # a mask bit at n_pdb
        expect(abi.E_STATE, lambda: e.preempt(m.pres))                               # a failed load leaves no table
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        e.preempt(m.pres)
        e.load_snapshot(m.table)                                                      # invalidates the table
        expect(abi.E_STATE, lambda: e.preempt(m.pres))


def test_reserve_pod_as_preemptor_is_einval(Engine):
    m = M.case("wave")
    pre = m.pres[:1].copy()
    pre["pod"]["flags"] |= abi.POD_RESERVE
    with loaded(Engine, m) as e:
        expect(abi.E_INVAL, lambda: e.preempt(pre))


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
        expect(abi.E_INVAL, lambda: e.preempt(m.pres))
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(m.pres[0]))
