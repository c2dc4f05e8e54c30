"""FitError reasons on a real MI355X against the CPU model (reasons_model.py),
bit for bit: koordhip_diagnose_reasons / koordhip_node_reasons (current
state), koordhip_fetch_reasons / koordhip_fetch_node_reasons (decision
states), the reference's Filter rows through the engine, the tie to the
existing status and koordhip_diag record, the lack of side effects and the
validity / envelope errors."""
import copy

import numpy as np
import pytest

import oracle
import reasons_model as RM
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config, with_deviceshare

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
    for f in ("feasible", "unresolvable", "first", "any"):
        if not np.array_equal(got[f], want[f]):
            bad = int(np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0])
            raise AssertionError(f"{f} differs first at pod {bad}: got {got[bad]} want {want[bad]}")


def assert_tied(rec, diag, masks, status, n):
    """One pod's reasons record and mask row against its status row and koordhip_diag record."""
    assert np.array_equal(abi.reasons_status(masks), status.astype(np.uint32))
    assert_records_equal(rec[None], RM.records(masks))
    first = abi.first_reasons(masks)
    assert rec["unresolvable"] == ((first & np.uint32(abi.REASON_UNRESOLVABLE_MASK)) != 0).sum()
    assert rec["feasible"] == diag["feasible"]
    for bit, group in abi.REASONS_OF_BIT.items():
        slots = [r for r in range(abi.REASON_SLOTS) if (group >> r) & 1]
        b = bit.bit_length() - 1
        if bit == abi.ST_FIT_FAIL:      # a node counts once in the plugin's slot, once per failing resource here
            assert rec["first"][slots].max() <= diag["first"][b] <= rec["first"][slots].sum()
            assert rec["any"][slots].max() <= diag["any"][b] <= rec["any"][slots].sum()
        else:
            assert rec["first"][slots].sum() == diag["first"][b], bit
            assert rec["any"][slots].sum() == diag["any"][b], bit
    assert not rec["first"][abi.REASON_COUNT:].any() and not rec["any"][abi.REASON_COUNT:].any()
    assert rec["feasible"] + (first != 0).sum() == n


# ------------------------------------------------- 1. the current state
def run_current(Engine, prof, table, pods):
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        rec = e.diagnose_reasons(pods)
        masks = np.stack([e.node_reasons(pods[p]) for p in range(len(pods))])
        diag = e.diagnose(pods)
        status = e.eval(pods, scores=False)["status"]
    for p in range(len(pods)):
        assert_tied(rec[p], diag[p], masks[p], status[p], table.n)
    return rec, masks


@pytest.mark.parametrize("name", RM.CURRENT_CASES)
def test_diagnose_reasons_is_the_model(Engine, name):
    """One lane, a partial wave, a ragged last node tile with three pod tiles;
    NodeNUMAResource; amplified, topology-policy and statically filtered nodes."""
    prof, table, pods = RM.current_case(name)
    want = RM.masks(oracle.Oracle(to_c_config(prof), table), pods)
    rec, masks = run_current(Engine, prof, table, pods)
    assert np.array_equal(masks, want)
    assert_records_equal(rec, RM.records(want))


def test_diagnose_reasons_reservation_snapshot(Engine):
    """Fit on the restored rows has no model: the structure, the Reservation
    reasons against the model's, and the tie to the status."""
    prof, table, pods = RM.resv_case()
    rec, masks = run_current(Engine, prof, table, pods)
    o = oracle.Oracle(to_c_config(prof), table)
    st = o.eval(pods, status=True, scores=False)["status"].astype(np.uint32)
    fit, resv = abi.REASONS_OF_BIT[abi.ST_FIT_FAIL], abi.REASONS_OF_BIT[abi.ST_RESV_FAIL]
    seen = 0
    for p in range(len(pods)):
        m = masks[p]
        assert np.array_equal((m & np.uint32(fit)) != 0, (st[p] & abi.ST_FIT_FAIL) != 0)
        r = m & np.uint32(resv)
        assert np.array_equal(r != 0, (st[p] & abi.ST_RESV_FAIL) != 0)
        assert ((r & (r - np.uint32(1))) == 0).all()                  # exactly one of the two
        if not pods["flags"][p] & abi.POD_RESV_AFFINITY:
            assert not (r & np.uint32(1 << abi.REASON_RESV_AFFINITY)).any()
        assert np.array_equal(r, RM.resv_mask(o, pods[p], st[p] & abi.ST_RESV_FAIL))
        seen |= int(np.bitwise_or.reduce(r))
    assert seen == resv


ROWS = RM.fixture_rows()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_fixture_row(Engine, row):
    _, w, bit, prof, t, pod = row
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        m = e.node_reasons(pod[0])
        rec = e.diagnose_reasons(pod)[0]
    RM.check_fixture_row(w, bit, m[0])
    assert_records_equal(rec[None], RM.records(m))


# ------------------------------------------------- 2. the decision states
@pytest.mark.parametrize("name,batch", [("A", 0), ("A", 17), ("C", 0)])
def test_fetch_reasons_is_the_decision_state(Engine, name, batch):
    m = RM.case(name)
    d = m.d
    picks = [int(d.unplaced[0]), int(d.unplaced[len(d.unplaced) // 2]), int(d.unplaced[-1]), int(m.differ[0])]
    with Engine(with_batch(d.prof, batch), device=0) as e:
        e.load_snapshot(d.table)
        out = e.place_stream(d.pods)
        got = e.fetch_reasons(len(d.pods))
        diag = e.fetch_diagnosis(len(d.pods))
        node = {u: (e.fetch_node_reasons(u), e.fetch_node_status(u)) for u in picks}
        final = e.diagnose_reasons(d.pods[d.unplaced])
        placed = int(np.flatnonzero(d.out >= 0)[0])
        with pytest.raises(abi.KoordhipError) as ei:
            e.fetch_node_reasons(placed)
        assert ei.value.code == abi.E_INVAL
    assert np.array_equal(out, d.out)
    assert_records_equal(got, m.rec)
    assert_records_equal(final, m.final_rec[d.unplaced])
    assert len(m.differ) and all(got[u] != m.final_rec[u] for u in m.differ)
    for u in picks:
        assert np.array_equal(node[u][0], m.mask[u]), u
        assert_tied(got[u], diag[u], node[u][0], node[u][1], d.table.n)


def test_fetch_reasons_prefix(Engine):
    m = RM.case("A")
    k = int(m.d.unplaced[len(m.d.unplaced) // 2]) + 1
    with Engine(m.d.prof, device=0) as e:
        e.load_snapshot(m.d.table)
        e.place_stream(m.d.pods)
        got = e.fetch_reasons(k)
    assert_records_equal(got, m.rec[:k])


def test_kinds_interleaved_share_the_workspaces(Engine):
    """The six calls of both kinds on one engine, twice round: they share the
    record and list workspaces, whose sizes follow the kind (264-B then 136-B
    records, 4-B then 1-B planes), so a small answer follows a large one."""
    m = RM.case("A")
    d = m.d
    u = int(d.unplaced[len(d.unplaced) // 2])
    up = d.pods[d.unplaced]
    with Engine(d.prof, device=0) as e:
        e.load_snapshot(d.table)
        e.place_stream(d.pods)
        rounds = [(e.fetch_reasons(len(d.pods)), e.fetch_diagnosis(len(d.pods)), e.fetch_node_reasons(u),
                   e.fetch_node_status(u), e.diagnose_reasons(up), e.diagnose(up)) for _ in range(2)]
    for got, diag, mask, status, final, final_diag in rounds:
        assert_records_equal(got, m.rec)
        assert np.array_equal(mask, m.mask[u])
        assert np.array_equal(status, d.status[u])
        assert_records_equal(final, m.final_rec[d.unplaced])
        for f in ("feasible", "any", "first"):
            assert np.array_equal(diag[f], d.rec[f]), f
            assert np.array_equal(final_diag[f], d.final_rec[d.unplaced][f]), f
    for a, b in zip(*rounds):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------- 3. no side effects
def test_reasons_change_no_state(Engine):
    m = RM.case("C")
    d = m.d
    with Engine(d.prof, device=0) as e:
        e.load_snapshot(d.table)
        e.place_stream(d.pods)
        n0, u0 = e.read_nodes(), e.read_numa()
        e.fetch_reasons(len(d.pods))
        e.fetch_node_reasons(int(d.unplaced[-1]))
        e.diagnose_reasons(d.pods[:40])
        e.node_reasons(d.pods[0])
        n1, u1 = e.read_nodes(), e.read_numa()
        later = e.fetch_diagnosis(len(d.pods))          # the place call is still there to diagnose
    for k in n0:
        assert n0[k].tobytes() == n1[k].tobytes(), k
    for k in u0:
        assert u0[k].tobytes() == u1[k].tobytes(), k
    for f in ("feasible", "any", "first"):
        assert np.array_equal(later[f], d.rec[f]), f


# ------------------------------------------------- 4. validity and envelope
def test_fetch_reasons_after_commit_is_estate(Engine):
    d = RM.case("A").d
    with Engine(d.prof, device=0) as e:
        e.load_snapshot(d.table)
        with pytest.raises(abi.KoordhipError) as ei:      # no place call yet
            e.fetch_reasons(1)
        assert ei.value.code == abi.E_STATE
        out = e.place_stream(d.pods)
        e.fetch_reasons(len(d.pods))
        j = int(np.flatnonzero(out >= 0)[0])
        e.commit(d.pods[j], int(out[j]))
        for call in (lambda: e.fetch_reasons(len(d.pods)), lambda: e.fetch_node_reasons(int(d.unplaced[0]))):
            with pytest.raises(abi.KoordhipError) as ei:
                call()
            assert ei.value.code == abi.E_STATE
        e.diagnose_reasons(d.pods[:3])                    # the current-state calls answer after a commit


def test_reasons_sequential_profile_is_einval(Engine):
    prof = with_deviceshare(shipped_profile())
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    synth.add_devices(table, synth.DevSpec())
    pods = synth.make_pods(synth.StreamSpec(4), prof)
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        for call in (lambda: e.diagnose_reasons(pods), lambda: e.node_reasons(pods[0])):
            with pytest.raises(abi.KoordhipError) as ei:
                call()
            assert ei.value.code == abi.E_INVAL


def test_reasons_reserve_pod_is_einval(Engine):
    prof, table, pods = RM.resv_case()
    reserve = pods[:2].copy()
    reserve["flags"] = (reserve["flags"] & ~np.uint32(abi.POD_RESV_AFFINITY)) | abi.POD_RESERVE
    reserve["resv_match"] = 0
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        for call in (lambda: e.diagnose_reasons(reserve), lambda: e.node_reasons(reserve[0])):
            with pytest.raises(abi.KoordhipError) as ei:
                call()
            assert ei.value.code == abi.E_INVAL
        out = e.place_stream(pods)
        with pytest.raises(abi.KoordhipError) as ei:      # Reservation plugin state: outside the replay's envelope
            e.fetch_reasons(len(pods))
        assert ei.value.code == abi.E_INVAL
        assert np.array_equal(e.fetch_placements(len(pods)), out)
