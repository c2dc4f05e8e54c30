"""Unschedulable-pod diagnosis on a real MI355X against the CPU oracle, bit for
bit: koordhip_diagnose (the histogram of koordhip_eval's status),
koordhip_fetch_diagnosis / koordhip_fetch_node_status (the unplaced pods of a
stream at the state each was decided on, diag_model.py), their lack of side
effects, and the validity / envelope errors."""
import copy

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config, with_deviceshare

import diag_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def with_batch(prof, batch):
    p = copy.deepcopy(prof)
    p.batch_pods = batch
    return p


def assert_records_equal(got, want):
    for f in ("feasible", "any", "first"):
        if not np.array_equal(got[f], want[f]):
            bad = int(np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0])
            raise AssertionError(f"{f} differs first at pod {bad}: got {got[bad]} want {want[bad]}")
    assert not got["reserved"].any()


# ------------------------------------------------------------ 1. diagnose
def check_diagnose(Engine, prof, table, pods):
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        got = e.diagnose(pods)
    ref = oracle.Oracle(to_c_config(prof), table).eval(pods, status=True, scores=False)["status"]
    assert_records_equal(got, M.records(ref))
    assert (got["feasible"] + got["first"].sum(axis=1) == table.n).all()


@pytest.mark.parametrize("n,n_pods", [(1, 3), (63, 7), (1003, 70)])
def test_diagnose_base_profile(Engine, n, n_pods):
    """One lane, a partial wave, a ragged last node tile with more than one pod tile."""
    prof = shipped_profile()
    table = synth.make_cluster(synth.ClusterSpec(n), prof)
    pods = synth.make_pods(synth.StreamSpec(n_pods, be_frac=0.3), prof)
    pods["flags"][::3] |= abi.POD_DAEMONSET
    check_diagnose(Engine, prof, table, pods)


def test_diagnose_numa(Engine):
    m = M.case("C")
    check_diagnose(Engine, m.prof, m.table, m.pods[:70])


def test_diagnose_reservation_snapshot(Engine):
    prof = shipped_profile(numa=True, reservation=True)
    table = synth.make_cluster(synth.ClusterSpec(400), prof)
    synth.add_numa(table, synth.NumaSpec(), prof)
    synth.add_reservations(table, synth.ResvSpec())
    pods = synth.make_pods(synth.StreamSpec(40, be_frac=0.3, cpuset_frac=0.3, resv_match_frac=0.3), prof)
    check_diagnose(Engine, prof, table, pods)


# ---------------------------------------------------- 2. fetch_diagnosis
@pytest.mark.parametrize("name,batch", [(c, b) for c in ("A", "B", "C") for b in M.BATCHES[c]])
def test_fetch_diagnosis_is_the_decision_state(Engine, name, batch):
    m = M.case(name)
    with Engine(with_batch(m.prof, batch), device=0) as e:
        e.load_snapshot(m.table)
        out = e.place_stream(m.pods)
        got = e.fetch_diagnosis(len(m.pods))
    assert np.array_equal(out, m.out)
    assert_records_equal(got, m.rec)


def test_fetch_diagnosis_prefix(Engine):
    """Fewer records than pods: the commits of the pods past the prefix are un-applied all the same."""
    m = M.case("B")
    k = int(m.unplaced[len(m.unplaced) // 2]) + 1
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        e.place_stream(m.pods)
        got = e.fetch_diagnosis(k)
    assert_records_equal(got, m.rec[:k])


# -------------------------------------------------- 3. fetch_node_status
@pytest.mark.parametrize("name", ["A", "C"])
def test_fetch_node_status(Engine, name):
    m = M.case(name)
    picks = [int(m.unplaced[0]), int(m.unplaced[len(m.unplaced) // 2]), int(m.unplaced[-1])]
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        e.place_stream(m.pods)
        got = {u: e.fetch_node_status(u) for u in picks}
        placed = int(np.flatnonzero(m.out >= 0)[0])
        with pytest.raises(abi.KoordhipError) as ei:
            e.fetch_node_status(placed)
        assert ei.value.code == abi.E_INVAL
    for u in picks:
        assert np.array_equal(got[u], m.status[u]), u


# ------------------------------------------------------ 4. no side effects
def test_fetch_diagnosis_changes_no_state(Engine):
    m = M.case("C")
    prof, cfg = m.prof, m.cfg
    more = synth.make_pods(synth.StreamSpec(120, be_frac=0.4, seed=7, cpuset_frac=0.5), prof)
    with Engine(prof, device=0) as e:
        e.load_snapshot(m.table)
        e.place_stream(m.pods)
        n0, u0 = e.read_nodes(), e.read_numa()
        e.fetch_diagnosis(len(m.pods))
        e.fetch_node_status(int(m.unplaced[-1]))
        n1, u1 = e.read_nodes(), e.read_numa()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        for k in u0:
            assert u0[k].tobytes() == u1[k].tobytes(), k
        for k in m.final_state:
            assert np.array_equal(n1[k], m.final_state[k]), k
        again = e.place_stream(more)
    o = oracle.Oracle(cfg, m.table)
    o.place_stream(m.pods)
    assert np.array_equal(again, o.place_stream(more))


# ------------------------------------------------- 5. validity and envelope
def test_abi_version_15():
    assert abi.KOORDHIP_ABI_VERSION == 15
    assert abi.load_library().koordhip_abi_version() == 15


def test_fetch_diagnosis_after_commit_is_estate(Engine):
    m = M.case("B")
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        with pytest.raises(abi.KoordhipError) as ei:      # no place call yet
            e.fetch_diagnosis(1)
        assert ei.value.code == abi.E_STATE
        out = e.place_stream(m.pods)
        e.fetch_diagnosis(len(m.pods))
        j = int(np.flatnonzero(out >= 0)[0])
        e.commit(m.pods[j], int(out[j]))
        for call in (lambda: e.fetch_diagnosis(len(m.pods)), lambda: e.fetch_node_status(int(m.unplaced[0]))):
            with pytest.raises(abi.KoordhipError) as ei:
                call()
            assert ei.value.code == abi.E_STATE


def test_fetch_diagnosis_reservation_stream_is_einval(Engine):
    prof = shipped_profile(numa=True, reservation=True)
    table = synth.make_cluster(synth.ClusterSpec(300), prof)
    synth.add_numa(table, synth.NumaSpec(), prof)
    synth.add_reservations(table, synth.ResvSpec())
    pods = synth.make_pods(synth.StreamSpec(200, be_frac=0.3, cpuset_frac=0.3, resv_match_frac=0.3), prof)
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        out = e.place_stream(pods)
        with pytest.raises(abi.KoordhipError) as ei:
            e.fetch_diagnosis(len(pods))
        assert ei.value.code == abi.E_INVAL
        assert np.array_equal(e.fetch_placements(len(pods)), out)
    assert np.array_equal(out, oracle.Oracle(to_c_config(prof), table).place_stream(pods))


def test_diagnose_sequential_profile_is_einval(Engine):
    prof = with_deviceshare(shipped_profile())
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    synth.add_devices(table, synth.DevSpec())
    pods = synth.make_pods(synth.StreamSpec(4), prof)
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        with pytest.raises(abi.KoordhipError) as ei:
            e.diagnose(pods)
        assert ei.value.code == abi.E_INVAL
