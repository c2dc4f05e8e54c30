"""The sequential preemption dry run under Reservation
(koordhip_preempt_stream_resv in the KOORDHIP_PREEMPT_RESV mode) on a real
MI355X against the plain-Python model (preempt_resv_stream_model.py), byte for
byte: the result records, the victims and the three stats counters; the
model's second form on the device (koordhip_preempt on reloaded, rebuilt
tables); the lack of side effects and the refusals."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, with_deviceshare, with_topology_spread

import preempt_dev_stream_model as DS
import preempt_model as M
import preempt_resv_model as V
import preempt_resv_stream_model as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def numa_of(m):
    return bool(int(m.cfg.filter_plugins) & abi.PLUGIN_NUMA)


def loaded(Engine, m, resv=True, numa_frozen=None, table=None):
    e = Engine(m.prof, device=0)
    e.preempt_set_mode(numa_frozen=numa_of(m) if numa_frozen is None else numa_frozen, resv=resv)
    e.load_snapshot(m.table if table is None else table)
    e.preempt_load_pods(m.assigned, m.pdb_allowed)
    return e


def assert_records_equal(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what} differs first at {bad}: got {got.reshape(-1)[bad]} want {want.reshape(-1)[bad]}")


def expect(code, call, match=None):
    with pytest.raises(abi.KoordhipError, match=match) as ei:
        call()
    assert ei.value.code == code, ei.value


# ------------------------------------------- 1. records, victims, stats: the model
@pytest.mark.parametrize("name", T.ALL_CASES)
def test_stream_against_the_model(Engine, name):
    """One lane; a wave with a second block; a second node block and a second
    preemptor tile on four slots with a list past 64 pods; the shipped profile
    on one slot and on four; ascending priorities; the hand-worked cases.
    max_victims exact, 0 and 1."""
    m = T.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(m.pres, max_victims=exact, resv=True)
        res0, vic0, st0 = e.preempt_stream(m.pres, max_victims=0, resv=True)
        res1, vic1, st1 = e.preempt_stream(m.pres, max_victims=1, resv=True)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert st == m.stats, name
    assert_records_equal(res0, m.res, f"{name}: results without victims")
    assert vic0.shape == (len(m.pres), 0) and st0 == m.stats
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    assert st1 == m.stats
    if name in T.EXPECTED:
        got = [(int(res["node"][k]), [int(j) for j in vic[k] if j >= 0]) for k in range(len(m.pres))]
        assert got == T.EXPECTED[name]


@pytest.mark.parametrize("name", ["wave", "numa4"])
def test_one_preemptor_is_preempt(Engine, name):
    """One slot (k_preempt_seq<false, 1>) and four with the frozen plane (k_preempt_seq<true, 4>)."""
    m = T.case(name)
    with loaded(Engine, m) as e:
        for p in range(len(m.pres)):
            res, vic, _ = e.preempt_stream(m.pres[p:p + 1], max_victims=4, resv=True)
            res1, vic1 = e.preempt(m.pres[p:p + 1], max_victims=4)
            assert_records_equal(res, res1, f"preemptor {p}: result")
            assert_records_equal(vic, vic1, f"preemptor {p}: victims")


# ------------------------------------------- 2. the model's second form on the device
def test_rebuilt_tables_on_the_device(Engine):
    """`ascending`: no preemptor sees an earlier one, so the rebuilt table says all of S_k.  For the preemptors with
    a gone bound pod before them, koordhip_preempt in the RESV mode on a context reloaded with that table is the
    stream's record and victims."""
    m = T.case("ascending")
    assert not any(m.sees_nominated)
    ks = [k for k in range(1, len(m.pres)) if m.gone_bound[k]]
    assert len(ks) >= 2
    with loaded(Engine, m) as e:
        res, vic, _ = e.preempt_stream(m.pres, max_victims=8, resv=True)
    nodes = [int(x) for x in res["node"]]
    chosen = [[int(j) for j in v if j >= 0] for v in vic]
    assert max(len(c) for c in chosen) < 8
    for k in ks:
        t, a_k, allowed, pre, keep, _ = T.rebuilt_inputs(m.table, m.assigned, m.pdb_allowed, m.pres, k, chosen, nodes)
        with Engine(m.prof, device=0) as e:
            e.preempt_set_mode(resv=True)
            e.load_snapshot(t)
            e.preempt_load_pods(a_k, allowed)
            r, v = e.preempt(pre, max_victims=8)
        assert_records_equal(r[0], res[k], f"preemptor {k}: result on the rebuilt table")
        assert [int(keep[j]) for j in v[0] if j >= 0] == chosen[k], f"preemptor {k}: victims on the rebuilt table"


# ------------------------------------------------------- 3. no side effects
def test_stream_changes_no_state(Engine):
    m = T.case("tiles")
    d = V.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, resv_match_frac=0.5, resv_groups=V.GROUPS, seed=11), m.prof)
    with loaded(Engine, m) as e:
        n0, r0 = e.read_nodes(), e.read_reservations()
        e.preempt_stream(m.pres, max_victims=4, resv=True)
        n1, r1 = e.read_nodes(), e.read_reservations()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        for k in r0:
            assert r0[k].tobytes() == r1[k].tobytes(), k
        res, vic = e.preempt(m.pres, max_victims=4)               # the loaded table is as it was
        after = e.place_stream(stream)
    assert_records_equal(res, d.res, "the independent batch after the stream")
    assert_records_equal(vic, M.victims_array(d.chosen, 4), "its victims")
    assert np.array_equal(after, oracle.Oracle(m.cfg, m.table).place_stream(stream))


# ------------------------------------------------------------ 4. the refusals
def test_refused_without_the_flag_or_the_state(Engine):
    m = T.case("wave")
    d = V.case("wave")
    with loaded(Engine, m, resv=False) as e:                       # the flag is missing
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True), match="KOORDHIP_PREEMPT_RESV")
        e.preempt_set_mode(resv=True)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream_resv")  # the plain call names it
        res, _ = e.preempt(m.pres)                                 # refused calls leave the context answering
        assert_records_equal(res, d.res, "koordhip_preempt after refused calls")
        with pytest.raises(ValueError):                            # the binding: not together with ext records
            e.preempt_stream(m.pres, ext=Engine.EXT_NULL, resv=True)
        res, _, st = e.preempt_stream(m.pres, resv=True)
    assert_records_equal(res, m.res, "results after refused calls")
    assert st == m.stats
    p = M.case("wave")                                             # Fit + LoadAware: no Reservation state
    with Engine(p.prof, device=0) as e:
        e.preempt_set_mode(resv=True)
        e.load_snapshot(p.table)
        e.preempt_load_pods(p.assigned, p.pdb_allowed)
        expect(abi.E_INVAL, lambda: e.preempt_stream(p.pres, resv=True), match="is koordhip_preempt_stream\\)")
        res, _ = e.preempt(p.pres)
    assert_records_equal(res, p.res, "the plain profile after a refused call")


def test_refused_numa_profiles(Engine):
    m = T.case("numa")
    d = V.case("numa")
    with loaded(Engine, m, resv=True, numa_frozen=False) as e:     # RESV alone keeps the NUMA refusal
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True), match="KOORDHIP_PREEMPT_NUMA_FROZEN")
    table = m.table.copy()                                         # both flags on a snapshot whose reservations hold CPUs
    synth.add_reserved_cpus(table, frac=1.0)
    with loaded(Engine, m, table=table) as e:
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True), match="resv_cpus")
    with loaded(Engine, m) as e:
        for flag in (abi.POD_RESERVE, abi.POD_RESV_OPERATING):     # reserve / operating-mode preemptors
            pres = m.pres.copy()
            pres["pod"]["flags"][1] |= flag
            expect(abi.E_INVAL, lambda: e.preempt_stream(pres, resv=True), match="reserve")
        res, _ = e.preempt(m.pres)
        assert_records_equal(res, d.res, "koordhip_preempt after refused calls")
        res, _, st = e.preempt_stream(m.pres, resv=True)
    assert_records_equal(res, m.res, "results after refused calls")
    assert st == m.stats


def test_refused_device_mode_and_sequential_cycle(Engine):
    m = T.case("wave")
    d = DS.case("wave")                                            # the DEVICE mode is set (a DeviceShare table)
    dprof = with_deviceshare(shipped_profile(reservation=True))
    with Engine(dprof, device=0) as e:
        e.preempt_set_mode(device=True, resv=True)
        e.load_snapshot(d.table)
        e.preempt_load_pods(d.assigned, d.pdb_allowed, ext=d.ax)
        expect(abi.E_INVAL, lambda: e.preempt_stream(d.pres, resv=True), match="KOORDHIP_PREEMPT_DEVICE")
    sprof = with_topology_spread(m.prof)                           # a sequential-cycle snapshot
    with Engine(sprof, device=0) as e:
        e.preempt_set_mode(resv=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True), match="sequential cycle")


def test_refused_with_a_communicator(Engine):
    m = T.case("wave")
    with loaded(Engine, m) as e:
        e.comm_init(Engine.comm_unique_id(), 1, 0)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True), match="communicator")
