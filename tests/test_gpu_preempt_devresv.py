"""The preemption dry run under DeviceShare beside Reservation state
(koordhip_preempt_set_mode with KOORDHIP_PREEMPT_DEVICE | KOORDHIP_PREEMPT_RESV |
KOORDHIP_PREEMPT_DEVICE_RESV, and KOORDHIP_PREEMPT_NUMA_FROZEN where
NodeNUMAResource filters) on a real MI355X against the plain-Python model
(preempt_devresv_model.py), byte for byte: the per-node verdicts,
koordhip_preempt_ext and its victims, the tie to the reasons diagnosis, the lack
of side effects, the mode word's rules and what stays refused."""
import numpy as np
import pytest

from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, with_deviceshare, with_interpod_affinity, with_topology_spread

import preempt_dev_model as D
import preempt_devresv_model as B
import preempt_model as M
import preempt_resv_model as V

pytestmark = pytest.mark.gpu

BOTH = abi.PREEMPT_DEVICE | abi.PREEMPT_RESV | abi.PREEMPT_DEVICE_RESV


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, m, table=None, prof=None):
    e = Engine(prof or m.prof, device=0)
    e.preempt_set_mode(numa_frozen=m.numa, resv=True, device=True, device_resv=True)
    e.load_snapshot(table if table is not None else m.table)
    e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
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


# ------------------------------------------------------------- 0. the opt-in
def test_the_word_is_accepted_and_answers(Engine):
    """The shipped profile with DeviceShare on a snapshot with cpu / memory reservations, device columns and
    bound device pods answers under all four flags."""
    m = B.case("numa1")
    assert m.numa and (m.assigned["flags"] & abi.ASG_RESV_SLOT_MASK).any() and m.ax["dev_slots"].any()
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(flags=BOTH | abi.PREEMPT_NUMA_FROZEN)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        res, _ = e.preempt(m.pres, ext=m.ext)
        ver = e.preempt_node_verdicts(m.pres[0], ext=m.ext[0])
    assert_records_equal(res, m.res, "results")
    assert_records_equal(ver, m.verdicts[0], "verdicts")


# ------------------------------------------------------- 1. per-node verdicts
@pytest.mark.parametrize("name", B.ALL_CASES)
def test_node_verdicts(Engine, name):
    """One lane; a full wave and a partial one; a second node tile and a second preemptor tile with eight device
    slots and a list of 128 pods; the frozen NUMA plane beside both states; each on one and on four reservation
    slots; the hand-worked cases."""
    m = B.case(name)
    picks = sorted({0, len(m.pres) // 2, len(m.pres) - 1})
    with loaded(Engine, m) as e:
        got = {p: e.preempt_node_verdicts(m.pres[p], ext=m.ext[p]) for p in picks}
    for p in picks:
        assert_records_equal(got[p], m.verdicts[p], f"{name}: verdicts of preemptor {p}")


@pytest.mark.parametrize("name", B.DIRECTED)
def test_directed_cases_as_written(Engine, name):
    m = B.case(name)
    with loaded(Engine, m) as e:
        ver = [e.preempt_node_verdicts(m.pres[p], ext=m.ext[p]) for p in range(len(m.pres))]
        res, vic = e.preempt(m.pres, max_victims=4, ext=m.ext)
    for p, want in enumerate(B.EXPECTED[name]):
        assert [int(s) for s in ver[p]["status"]] == [s for s, _ in want], p
        node = int(res["node"][p])
        cands = [i for i, (s, _) in enumerate(want) if s == abi.PREEMPT_CANDIDATE]
        assert (node in cands) if cands else node == -1
        if node >= 0:
            assert [int(v) for v in vic[p] if v >= 0] == want[node][1]


# ------------------------------------------------------ 2. results and victims
@pytest.mark.parametrize("name", B.ALL_CASES)
def test_preempt_results_and_victims(Engine, name):
    m = B.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic = e.preempt(m.pres, max_victims=exact, ext=m.ext)
        res0, vic0 = e.preempt(m.pres, max_victims=0, ext=m.ext)
        res1, vic1 = e.preempt(m.pres, max_victims=1, ext=m.ext)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert_records_equal(res0, m.res, f"{name}: results without victims")
    assert vic0.shape == (len(m.pres), 0)
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    assert (res["count"].sum(axis=1) == m.table.n).all()


def test_ext_none_is_zeroed_records(Engine):
    m = B.case("tiles4")
    zero = abi.pod_ext_array(len(m.pres))
    with loaded(Engine, m) as e:
        res_n, vic_n = e.preempt(m.pres, max_victims=3)
        res_z, vic_z = e.preempt(m.pres, max_victims=3, ext=zero)
        ver_n = e.preempt_node_verdicts(m.pres[4])
        ver_z = e.preempt_node_verdicts(m.pres[4], ext=zero[4])
    assert_records_equal(res_n, res_z, "results")
    assert_records_equal(vic_n, vic_z, "victims")
    assert_records_equal(ver_n, ver_z, "verdicts")
    want = B.dry_run(m.resv_cfg, m.table, m.assigned, m.pdb_allowed, m.pres[:6], zero[:6], m.ax, m.base_cfg)
    assert_records_equal(res_n[:6], want[0], "results against the model without requests")


@pytest.mark.parametrize("name", ["tiles1", "tiles4"])
def test_batch_of_non_device_preemptors(Engine, name):
    """No preemptor of the call has KOORDHIP_PODX_DEVICE: the walk without device state (DEV = 1), whose
    Reservation maps still carry the listed pods' scalars."""
    m = B.case(name)
    keep = np.flatnonzero((m.ext["flags"] & abi.PODX_DEVICE) == 0)
    assert len(keep) >= 2
    ext = m.ext[keep].copy()
    ext["xreq"][::2, B.KN], ext["xmask"][::2] = 1, 1 << B.KN
    pres = m.pres[keep]
    want = B.dry_run(m.resv_cfg, m.table, m.assigned, m.pdb_allowed, pres, ext, m.ax, m.base_cfg)
    with loaded(Engine, m) as e:
        res, vic = e.preempt(pres, max_victims=2, ext=ext)
        ver = e.preempt_node_verdicts(pres[0], ext=ext[0])
    assert_records_equal(res, want[0], "results")
    assert_records_equal(vic, M.victims_array(want[2], 2), "victims")
    assert_records_equal(ver, want[1][0], "verdicts")


# ---------------------------------- 3. UNRESOLVABLE against the reasons kernel
@pytest.mark.parametrize("name", ["tiles4", "numa1", "affinity_device"])
def test_unresolvable_count_is_the_diagnosis(Engine, name):
    m = B.case(name)
    with loaded(Engine, m) as e:
        res, _ = e.preempt(m.pres, ext=m.ext)
        rec = e.diagnose_reasons_ext(np.ascontiguousarray(m.pres["pod"]), m.ext)
    assert np.array_equal(res["count"][:, abi.PREEMPT_UNRESOLVABLE], rec["unresolvable"])
    assert rec["unresolvable"].any()


# ------------------------------------------------------- 4. no side effects
def test_dry_runs_change_no_state(Engine):
    m = B.case("tiles4")
    with loaded(Engine, m) as e:
        n0, d0, r0 = e.read_nodes(), e.read_devices(), e.read_reservations()
        e.preempt(m.pres, max_victims=4, ext=m.ext)
        e.preempt_node_verdicts(m.pres[0], ext=m.ext[0])
        n1, d1, r1 = e.read_nodes(), e.read_devices(), e.read_reservations()
    for before, after in ((n0, n1), (d0, d1), (r0, r1)):
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k


# ------------------------------------------------------------------ 5. the mode
def test_mode_words(Engine):
    m = B.case("wave1")
    with loaded(Engine, m) as e:
        for bits in (8, 8 | abi.PREEMPT_DEVICE, 8 | abi.PREEMPT_RESV, 16, BOTH | 16, 1 << 31):
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))     # ... and they leave the mode as it was
        res, _ = e.preempt(m.pres, ext=m.ext)
        assert_records_equal(res, m.res, "results after refused mode words")
        e.preempt_set_mode(flags=0)                                # set_mode(0) restores today's refusal
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext))
        e.preempt_set_mode(device=True, resv=True)                 # ... and so does the word without the opt-in
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="follow-up")
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(m.pres[0]), match="KOORDHIP_PREEMPT_RESV")
        e.preempt_set_mode(resv=True, device=True, device_resv=True)
        res, _ = e.preempt(m.pres, ext=m.ext)
    assert_records_equal(res, m.res, "results after the mode came back")
    for prof in (D.dev_profile(), V.resv_profile()):               # a profile lacking either plugin: like an unknown bit
        with Engine(prof, device=0) as e:
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=BOTH), match="KOORDHIP_PREEMPT_DEVICE_RESV")
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=BOTH | abi.PREEMPT_NUMA_FROZEN))
    d = D.case("wave")                                             # ... and that context's mode stayed what it was
    with Engine(d.prof, device=0) as e:
        e.preempt_set_mode(device=True)
        expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=BOTH))
        e.load_snapshot(d.table)
        e.preempt_load_pods(d.assigned, d.pdb_allowed, ext=d.ax)
        res, _ = e.preempt(d.pres, ext=d.ext)
    assert_records_equal(res, d.res, "the DEVICE mode after a refused word")


def test_numa_profiles_need_all_four(Engine):
    m = B.case("numa4")
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(resv=True, device=True, device_resv=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="KOORDHIP_PREEMPT_NUMA_FROZEN")


# ------------------------------------------------------------ 6. still refused
def test_streams_stay_refused(Engine):
    m = B.case("wave4")
    with loaded(Engine, m) as e:
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream: .*KOORDHIP_PREEMPT_DEVICE_RESV")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=m.ext),
               match="koordhip_preempt_stream_ext: .*KOORDHIP_PREEMPT_DEVICE_RESV")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=Engine.EXT_NULL), match="koordhip_preempt_stream_ext")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, resv=True),
               match="koordhip_preempt_stream_resv: .*KOORDHIP_PREEMPT_DEVICE_RESV")
        res, _ = e.preempt(m.pres, ext=m.ext)                      # a refused call leaves the context answering
    assert_records_equal(res, m.res, "results after refused streams")


def test_device_holding_reservations_stay_refused(Engine):
    m = B.case("wave4")
    t = m.table.copy()
    synth.add_device_reservations(t, synth.DevResvSpec())
    with loaded(Engine, m, table=t) as e:
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="resv_dev_slot")
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(m.pres[0], ext=m.ext[0]), match="tryAllocateFromReservation")
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        res, _ = e.preempt(m.pres, ext=m.ext)
    assert_records_equal(res, m.res, "results after a refused snapshot")


def test_more_slots_than_the_walk_holds_stay_refused(Engine):
    m = B.case("wave4")
    t = m.table.copy()
    t.set_resv_slots(abi.RESV_SLOTS + 1)                           # such a snapshot places in the sequential cycle
    with loaded(Engine, m, table=t) as e:
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="KOORDHIP_RESV_SLOTS")


def test_reserved_cpus_stay_refused_with_the_numa_flag(Engine):
    m = B.case("numa1")
    t = m.table.copy()
    synth.add_reserved_cpus(t, frac=1.0)
    assert any(t[f"resv_cpus{w}"].any() for w in range(abi.NUMA_WORDS))
    with loaded(Engine, m, table=t) as e:
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="resv_cpus")


def test_other_sequential_cycle_plugins_stay_refused(Engine):
    m = B.case("wave1")
    sprof = with_interpod_affinity(with_topology_spread(m.prof))
    with loaded(Engine, m, prof=sprof) as e:
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="PodTopologySpread")


def test_preemptors_that_stay_refused(Engine):
    m = B.case("numa1")
    with loaded(Engine, m) as e:
        for flag in (abi.POD_RESERVE, abi.POD_RESV_OPERATING):
            pre = m.pres[:1].copy()
            pre["pod"]["flags"] |= flag
            expect(abi.E_INVAL, lambda: e.preempt(pre, ext=m.ext[:1]), match="reserve")
        pre = m.pres[:1].copy()
        pre["pod"]["flags"] |= abi.POD_NUMA_ERROR
        expect(abi.E_INVAL, lambda: e.preempt(pre, ext=m.ext[:1]), match="KOORDHIP_POD_NUMA_ERROR")
        res, _ = e.preempt(m.pres, ext=m.ext)
    assert_records_equal(res, m.res, "results after refused preemptors")


def test_refused_with_a_communicator(Engine):
    m = B.case("wave1")
    with loaded(Engine, m) as e:
        e.comm_init(Engine.comm_unique_id(), 1, 0)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="communicator")
