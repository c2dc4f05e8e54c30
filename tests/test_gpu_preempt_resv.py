"""The preemption dry run under Reservation (koordhip_preempt_set_mode with
KOORDHIP_PREEMPT_RESV) on a real MI355X against the plain-Python model
(preempt_resv_model.py), bit for bit: the per-node verdicts, koordhip_preempt
and its victims, the tie to the reasons diagnosis, the lack of side effects
and the mode's errors."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile

import preempt_model as M
import preempt_numa_model as N
import preempt_resv_model as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def numa_of(m):
    return bool(int(m.cfg.filter_plugins) & abi.PLUGIN_NUMA)


def loaded(Engine, m, resv=True, numa_frozen=None):
    e = Engine(m.prof, device=0)
    e.preempt_set_mode(numa_frozen=numa_of(m) if numa_frozen is None else numa_frozen, resv=resv)
    e.load_snapshot(m.table)
    e.preempt_load_pods(m.assigned, m.pdb_allowed)
    return e


def assert_records_equal(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what} differs first at {bad}: got {got.reshape(-1)[bad]} want {want.reshape(-1)[bad]}")


def expect(code, call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == code, ei.value


# ------------------------------------------------------- 1. per-node verdicts
@pytest.mark.parametrize("name", V.ALL_CASES)
def test_node_verdicts(Engine, name):
    """One lane; two waves and a partial one; a second node tile and a second
    preemptor tile on four slots with lists past 64 pods; the shipped profile
    on one slot and on four (k_preempt<true, 4>, k_preempt_victims<true, 4>)."""
    m = V.case(name)
    picks = sorted({0, len(m.pres) // 2, len(m.pres) - 1})
    with loaded(Engine, m) as e:
        got = {p: e.preempt_node_verdicts(m.pres[p]) for p in picks}
    for p in picks:
        assert_records_equal(got[p], m.verdicts[p], f"{name}: verdicts of preemptor {p}")


# ------------------------------------------------------ 2. results and victims
@pytest.mark.parametrize("name", V.ALL_CASES)
def test_preempt_results_and_victims(Engine, name):
    m = V.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic = e.preempt(m.pres, max_victims=exact)
        res0, vic0 = e.preempt(m.pres, max_victims=0)
        res1, vic1 = e.preempt(m.pres, max_victims=1)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert_records_equal(res0, m.res, f"{name}: results without victims")
    assert vic0.shape == (len(m.pres), 0)
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    assert (res["count"].sum(axis=1) == m.table.n).all()


# ---------------------------------- 3. UNRESOLVABLE against the reasons kernel
@pytest.mark.parametrize("name", ["tiles", "numa"])
def test_unresolvable_count_is_the_diagnosis(Engine, name):
    """Cases with affinity preemptors: RESV_AFFINITY as the first failing plugin is unresolvable."""
    m = V.case(name)
    assert (m.pres["pod"]["flags"] & abi.POD_RESV_AFFINITY).any()
    with loaded(Engine, m) as e:
        res, _ = e.preempt(m.pres)
        rec = e.diagnose_reasons(np.ascontiguousarray(m.pres["pod"]))
    assert np.array_equal(res["count"][:, abi.PREEMPT_UNRESOLVABLE], rec["unresolvable"])
    assert rec["unresolvable"].any()


# ------------------------------------------------------- 4. no side effects
def test_dry_runs_change_no_state(Engine):
    m = V.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, resv_match_frac=0.5, resv_groups=V.GROUPS, seed=11), m.prof)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        plain = e.place_stream(stream)
    with loaded(Engine, m) as e:
        n0, r0 = e.read_nodes(), e.read_reservations()
        e.preempt(m.pres, max_victims=4)
        e.preempt_node_verdicts(m.pres[0])
        n1, r1 = e.read_nodes(), e.read_reservations()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        for k in r0:
            assert r0[k].tobytes() == r1[k].tobytes(), k
        after = e.place_stream(stream)
    assert np.array_equal(after, plain)
    assert np.array_equal(plain, oracle.Oracle(m.cfg, m.table).place_stream(stream))


# ------------------------------------------------------------------ 5. the mode
def test_mode_errors_and_lifetime(Engine):
    m = V.case("wave")
    calls = (lambda e: e.preempt(m.pres), lambda e: e.preempt_node_verdicts(m.pres[0]))
    with loaded(Engine, m, resv=False) as e:
        for call in calls:                                         # the default mode refuses
            expect(abi.E_INVAL, lambda: call(e))
        with pytest.raises(abi.KoordhipError, match="KOORDHIP_PREEMPT_RESV"):
            e.preempt(m.pres)
        e.preempt_set_mode(resv=True)
        for bits in (4, 6, 1 << 31):                               # unknown bits, and they leave the mode as it was
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))
        res, _ = e.preempt(m.pres)
        assert_records_equal(res, m.res, "results after refused mode words")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres))      # the stream: not with Reservation state, flag or not
        with pytest.raises(abi.KoordhipError, match="koordhip_preempt_stream"):
            e.preempt_stream(m.pres)
        res, _ = e.preempt(m.pres)                                 # a refused call leaves the context usable
        assert_records_equal(res, m.res, "results after a refused stream")
        e.preempt_set_mode(flags=0)                                # set_mode(0) restores the refusal
        for call in calls:
            expect(abi.E_INVAL, lambda: call(e))
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres))


def test_the_flag_is_inert_without_reservation_state(Engine):
    m = M.case("tiles")                                            # Fit + LoadAware: preempt_model's recorded answers
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(resv=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        res, vic = e.preempt(m.pres, max_victims=2)
        ver = e.preempt_node_verdicts(m.pres[5])
        sres, svic, _ = e.preempt_stream(m.pres, max_victims=2)    # the stream is not refused there either
    assert_records_equal(res, m.res, "results of preempt_model's tiles with the flag set")
    assert_records_equal(vic, M.victims_array(m.chosen, 2), "victims")
    assert_records_equal(ver, m.verdicts[5], "verdicts")
    assert sres.shape == res.shape and svic.shape == vic.shape


def test_resv_bit_is_refused_where_numa_filters_without_the_plugin(Engine):
    """NodeNUMAResource in the Filter and no Reservation plugin: the word is live and the context can never hold
    Reservation state, so a word with the bit is refused like an unknown one and the mode stays."""
    m = N.case("wave")
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(numa_frozen=True)
        for bits in (abi.PREEMPT_RESV, abi.PREEMPT_RESV | abi.PREEMPT_NUMA_FROZEN):
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        res, _ = e.preempt(m.pres)
    assert_records_equal(res, m.res, "the NUMA mode after refused words")


def test_numa_profiles_need_both_flags(Engine):
    m = V.case("numa")
    with loaded(Engine, m, resv=True, numa_frozen=False) as e:     # RESV alone keeps the NUMA refusal
        expect(abi.E_INVAL, lambda: e.preempt(m.pres))
        with pytest.raises(abi.KoordhipError, match="KOORDHIP_PREEMPT_NUMA_FROZEN"):
            e.preempt_node_verdicts(m.pres[0])
    with loaded(Engine, m, resv=False, numa_frozen=True) as e:     # NUMA_FROZEN alone keeps the Reservation refusal
        expect(abi.E_INVAL, lambda: e.preempt(m.pres))
    # both flags on a snapshot whose reservations hold CPUs
    table = m.table.copy()
    synth.add_reserved_cpus(table, frac=1.0)
    assert any(table[f"resv_cpus{w}"].any() for w in range(abi.NUMA_WORDS))
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(numa_frozen=True, resv=True)
        e.load_snapshot(table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres))
        with pytest.raises(abi.KoordhipError, match="resv_cpus"):
            e.preempt_node_verdicts(m.pres[0])


def test_slot_field_above_resv_slots_is_einval(Engine):
    m = V.case("wave")                                             # one slot per node
    a = m.assigned.copy()
    a["flags"][0] = (int(a["flags"][0]) & ~abi.ASG_RESV_SLOT_MASK) | abi.asg_resv_slot(1)
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(resv=True)
        e.load_snapshot(m.table)
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(a, m.pdb_allowed))
        e.preempt_load_pods(m.assigned, m.pdb_allowed)             # a refused table leaves the context usable
        res, _ = e.preempt(m.pres)
    assert_records_equal(res, m.res, "results after a refused table")
    p = M.case("wave")                                             # without reservation columns the field is ignored
    b = p.assigned.copy()
    b["flags"] |= abi.asg_resv_slot(7)
    with Engine(p.prof, device=0) as e:
        e.load_snapshot(p.table)
        e.preempt_load_pods(b, p.pdb_allowed)
        res, _ = e.preempt(p.pres)
    assert_records_equal(res, p.res, "results with ignored slot fields")


def test_reserve_and_operating_preemptors_stay_refused(Engine):
    m = V.case("wave")
    with loaded(Engine, m) as e:
        for flag in (abi.POD_RESERVE, abi.POD_RESV_OPERATING):
            pre = m.pres[:1].copy()
            pre["pod"]["flags"] |= flag
            expect(abi.E_INVAL, lambda: e.preempt(pre))
