"""The preemption dry run under NodeNUMAResource (koordhip_preempt_set_mode with
KOORDHIP_PREEMPT_NUMA_FROZEN) on a real MI355X against the oracle-only model
(preempt_numa_model.py), bit for bit: the per-node verdicts, koordhip_preempt,
koordhip_preempt_stream, the tie to the reasons diagnosis, the lack of side
effects and the mode's errors."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, with_deviceshare

import preempt_model as M
import preempt_numa_model as N

pytestmark = pytest.mark.gpu

STAT_KEYS = ("full_recomputes", "block_recomputes", "blocks_skipped")


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, m, frozen=True):
    e = Engine(m.prof, device=0)
    e.preempt_set_mode(numa_frozen=frozen)
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
@pytest.mark.parametrize("name", N.ALL_CASES)
def test_node_verdicts(Engine, name):
    """One lane, a partial wave, a last plane word of one bit and a second preemptor tile; 8 zones; static filters."""
    m = N.case(name)
    picks = sorted({0, len(m.pres) // 2, len(m.pres) - 1} | set(range(min(len(m.pres), 4))))
    with loaded(Engine, m) as e:
        got = {p: e.preempt_node_verdicts(m.pres[p]) for p in picks}
    for p in picks:
        assert_records_equal(got[p], m.verdicts[p], f"{name}: verdicts of preemptor {p}")


# ------------------------------------------------------ 2. results and victims
@pytest.mark.parametrize("name", N.ALL_CASES)
def test_preempt_results_and_victims(Engine, name):
    m = N.case(name)
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


@pytest.mark.parametrize("name", N.ALL_CASES)
def test_stream_results_victims_and_stats(Engine, name):
    m = N.stream_case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(m.pres, max_victims=exact)
        res1, vic1, st1 = e.preempt_stream(m.pres, max_victims=1)
    assert_records_equal(res, m.res, f"{name}: results")
    assert_records_equal(vic, M.victims_array(m.chosen, exact), f"{name}: victims")
    assert_records_equal(res1, m.res, f"{name}: results with a truncated list")
    assert_records_equal(vic1, M.victims_array(m.chosen, 1), f"{name}: truncated victims")
    for s in (st, st1):
        assert {k: s[k] for k in STAT_KEYS} == {k: m.stats[k] for k in STAT_KEYS}, name


@pytest.mark.parametrize("name", N.ALL_CASES)
def test_one_preemptor_both_ways(Engine, name):
    m = N.case(name)
    with loaded(Engine, m) as e:
        for p in sorted({0, len(m.pres) - 1}):
            one, onev = e.preempt(m.pres[p:p + 1], max_victims=4)
            res, vic, _ = e.preempt_stream(m.pres[p:p + 1], max_victims=4)
            assert_records_equal(res, one, f"{name}: preemptor {p} alone, stream against independent")
            assert_records_equal(vic, onev, f"{name}: preemptor {p} alone, victims")
            assert_records_equal(one, m.res[p:p + 1], f"{name}: preemptor {p} alone against the model")


# ------------------------------------- 3. the plane against the reasons kernel
@pytest.mark.parametrize("name", ["wave", "tiles"])
def test_unresolvable_count_is_the_diagnosis(Engine, name):
    """Two device code paths: k_preempt_numa's plane and filter_reasons."""
    m = N.case(name)
    with loaded(Engine, m) as e:
        res, _ = e.preempt(m.pres)
        rec = e.diagnose_reasons(np.ascontiguousarray(m.pres["pod"]))
    assert np.array_equal(res["count"][:, abi.PREEMPT_UNRESOLVABLE], rec["unresolvable"])
    assert rec["unresolvable"].any()


# ------------------------------------------------------- 4. no side effects
def test_dry_runs_change_no_state(Engine):
    m = N.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, cpuset_frac=0.3, seed=11), m.prof)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        plain = e.place_stream(stream)
    with loaded(Engine, m) as e:
        n0 = e.read_nodes()
        e.preempt(m.pres, max_victims=4)
        e.preempt_node_verdicts(m.pres[0])
        e.preempt_stream(m.pres, max_victims=4)
        n1 = e.read_nodes()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        after = e.place_stream(stream)
    assert np.array_equal(after, plain)
    assert np.array_equal(plain, oracle.Oracle(m.cfg, m.table).place_stream(stream))


# ------------------------------------------------------------------ 5. the mode
def test_mode_errors_and_lifetime(Engine):
    m = N.case("wave")
    calls = (lambda e: e.preempt(m.pres), lambda e: e.preempt_node_verdicts(m.pres[0]), lambda e: e.preempt_stream(m.pres))
    with loaded(Engine, m, frozen=False) as e:
        for call in calls:                                         # the default mode
            expect(abi.E_INVAL, lambda: call(e))
        with pytest.raises(abi.KoordhipError, match="koordhip_preempt_set_mode"):
            e.preempt(m.pres)
        e.preempt_set_mode(numa_frozen=True)
        for bits in (2, 3, 1 << 31):                               # unknown bits, and they leave the mode as it was
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))
        res, _ = e.preempt(m.pres)
        assert_records_equal(res, m.res, "results after refused mode words")
        e.load_snapshot(m.table)                                   # the mode outlives a snapshot and a table
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        res, _ = e.preempt(m.pres)
        assert_records_equal(res, m.res, "results after a reload")
        e.preempt_set_mode(numa_frozen=False)
        for call in calls:
            expect(abi.E_INVAL, lambda: call(e))


def test_numa_error_preemptor_is_einval(Engine):
    m = N.case("wave")
    pre = m.pres.copy()
    pre["pod"]["flags"][1] |= abi.POD_NUMA_ERROR
    with loaded(Engine, m) as e:
        expect(abi.E_INVAL, lambda: e.preempt(pre))
        expect(abi.E_INVAL, lambda: e.preempt_stream(pre))
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(pre[1]))
        res, _ = e.preempt(m.pres)                                 # a refused call leaves the context usable
    assert_records_equal(res, m.res, "results after refused calls")


@pytest.mark.parametrize("kind", ["reservation", "numa+reservation", "sequential"])
def test_the_rest_of_the_envelope_stays(Engine, kind):
    prof = {"reservation": lambda: shipped_profile(reservation=True),
            "numa+reservation": lambda: shipped_profile(numa=True, reservation=True),
            "sequential": lambda: with_deviceshare(shipped_profile(numa=True))}[kind]()
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    synth.add_numa(table, synth.NumaSpec(), prof)
    if "reservation" in kind:
        synth.add_reservations(table, synth.ResvSpec())
    if kind == "sequential":
        synth.add_devices(table, synth.DevSpec())
    m = M.case("wave")
    with Engine(prof, device=0) as e:
        e.preempt_set_mode(numa_frozen=True)
        e.load_snapshot(table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres))
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(m.pres[0]))
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres))
    pre = m.pres[:1].copy()
    pre["pod"]["flags"] |= abi.POD_RESERVE
    w = N.case("wave")
    with loaded(Engine, w) as e:
        expect(abi.E_INVAL, lambda: e.preempt(pre))


def test_the_flag_is_inert_without_numa(Engine):
    m = M.case("tiles")
    with loaded(Engine, m) as e:
        res, vic = e.preempt(m.pres, max_victims=2)
        ver = e.preempt_node_verdicts(m.pres[5])
    assert_records_equal(res, m.res, "results of preempt_model's tiles with the flag set")
    assert_records_equal(vic, M.victims_array(m.chosen, 2), "victims")
    assert_records_equal(ver, m.verdicts[5], "verdicts")
