"""The preemption dry run under DeviceShare (koordhip_preempt_set_mode with
KOORDHIP_PREEMPT_DEVICE) on a real MI355X against the plain-Python model
(preempt_dev_model.py), byte for byte: the per-node verdicts, koordhip_preempt_ext
and its victims, the tie to the reasons diagnosis, the lack of side effects,
the mode's errors and the refused tables."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import (shipped_profile, with_deviceshare, with_interpod_affinity, with_topology_spread)

import preempt_dev_model as D
import preempt_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, m, device=True, ax=True):
    e = Engine(m.prof, device=0)
    e.preempt_set_mode(numa_frozen=m.numa, device=device)
    e.load_snapshot(m.table)
    e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax if ax else None)
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


# ------------------------------------------------------- 1. per-node verdicts
@pytest.mark.parametrize("name", D.ALL_CASES)
def test_node_verdicts(Engine, name):
    """One lane; a full wave and a partial one; a second node tile and a second
    preemptor tile with eight device slots and a list past 64 pods; the frozen
    NUMA plane beside the device state; the hand-worked cases."""
    m = D.case(name)
    picks = sorted({0, len(m.pres) // 2, len(m.pres) - 1})
    with loaded(Engine, m) as e:
        got = {p: e.preempt_node_verdicts(m.pres[p], ext=m.ext[p]) for p in picks}
    for p in picks:
        assert_records_equal(got[p], m.verdicts[p], f"{name}: verdicts of preemptor {p}")


@pytest.mark.parametrize("name", D.DIRECTED)
def test_directed_cases_as_written(Engine, name):
    m = D.case(name)
    with loaded(Engine, m) as e:
        ver = e.preempt_node_verdicts(m.pres[0], ext=m.ext[0])
        res, vic = e.preempt(m.pres, max_victims=4, ext=m.ext)
    want = D.EXPECTED[name]
    assert [int(s) for s in ver["status"]] == [s for s, _ in want]
    node = int(res["node"][0])
    cands = [i for i, (s, _) in enumerate(want) if s == abi.PREEMPT_CANDIDATE]
    assert (node in cands) if cands else node == -1
    if node >= 0:
        assert [int(v) for v in vic[0] if v >= 0] == want[node][1]


# ------------------------------------------------------ 2. results and victims
@pytest.mark.parametrize("name", D.ALL_CASES)
def test_preempt_results_and_victims(Engine, name):
    m = D.case(name)
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
    """The plain calls in the DEVICE mode are the _ext calls with all-empty records (state.skip)."""
    m = D.case("tiles")
    zero = abi.pod_ext_array(len(m.pres))
    with loaded(Engine, m) as e:
        res_n, vic_n = e.preempt(m.pres, max_victims=3)
        res_z, vic_z = e.preempt(m.pres, max_victims=3, ext=zero)
        ver_n = e.preempt_node_verdicts(m.pres[4])
        ver_z = e.preempt_node_verdicts(m.pres[4], ext=zero[4])
    assert_records_equal(res_n, res_z, "results")
    assert_records_equal(vic_n, vic_z, "victims")
    assert_records_equal(ver_n, ver_z, "verdicts")
    want = D.dry_run(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres[:6], zero[:6], m.ax)
    assert_records_equal(res_n[:6], want[0], "results against the model without requests")


def test_batch_of_non_device_preemptors(Engine):
    """No preemptor of the call has KOORDHIP_PODX_DEVICE: the scalars-only walk (DEV = 1)."""
    m = D.case("tiles")
    keep = np.flatnonzero((m.ext["flags"] & abi.PODX_DEVICE) == 0)
    assert len(keep) >= 2
    # ... some of them with a scalar request, so that the second table is read
    ext = m.ext[keep].copy()
    k = D.XRES_INDEX[D.NVIDIA_GPU]
    ext["xreq"][::2, k], ext["xmask"][::2] = 1, 1 << k
    pres = m.pres[keep]
    want = D.dry_run(m.base_cfg, m.table, m.assigned, m.pdb_allowed, pres, ext, m.ax)
    with loaded(Engine, m) as e:
        res, vic = e.preempt(pres, max_victims=2, ext=ext)
        ver = e.preempt_node_verdicts(pres[0], ext=ext[0])
    assert_records_equal(res, want[0], "results")
    assert_records_equal(vic, M.victims_array(want[2], 2), "victims")
    assert_records_equal(ver, want[1][0], "verdicts")


# ---------------------------------- 3. UNRESOLVABLE against the reasons kernel
@pytest.mark.parametrize("name", ["tiles", "numa"])
def test_unresolvable_count_is_the_diagnosis(Engine, name):
    m = D.case(name)
    with loaded(Engine, m) as e:
        res, _ = e.preempt(m.pres, ext=m.ext)
        rec = e.diagnose_reasons_ext(np.ascontiguousarray(m.pres["pod"]), m.ext)
    assert np.array_equal(res["count"][:, abi.PREEMPT_UNRESOLVABLE], rec["unresolvable"])
    if name == "numa":
        assert rec["unresolvable"].any()


# ------------------------------------------------------- 4. no side effects
def test_dry_runs_change_no_state(Engine):
    m = D.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, seed=11), m.prof)
    sext = synth.make_device_ext(150, synth.DevStreamSpec(frac=0.3))
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        plain = e.place_stream_ext(stream, sext)
    with loaded(Engine, m) as e:
        n0, d0 = e.read_nodes(), e.read_devices()
        e.preempt(m.pres, max_victims=4, ext=m.ext)
        e.preempt_node_verdicts(m.pres[0], ext=m.ext[0])
        n1, d1 = e.read_nodes(), e.read_devices()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        for k in d0:
            assert d0[k].tobytes() == d1[k].tobytes(), k
        after = e.place_stream_ext(stream, sext)
    assert np.array_equal(after, plain)
    assert np.array_equal(plain, oracle.Oracle(m.cfg, m.table).place_stream_ext(stream, sext))


# ------------------------------------------------------------------ 5. the mode
def test_mode_errors_and_lifetime(Engine):
    m = D.case("wave")
    calls = (lambda e: e.preempt(m.pres), lambda e: e.preempt_node_verdicts(m.pres[0]),
             lambda e: e.preempt(m.pres, ext=m.ext), lambda e: e.preempt_node_verdicts(m.pres[0], ext=m.ext[0]))
    with loaded(Engine, m, device=False) as e:                      # a fresh context's mode
        for call in calls[:2]:
            expect(abi.E_INVAL, lambda: call(e), match="KOORDHIP_PREEMPT_DEVICE")
        for call in calls[2:]:                                     # ext records outside the mode
            expect(abi.E_INVAL, lambda: call(e))
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream")
        e.preempt_set_mode(flags=abi.PREEMPT_DEVICE)
        for bits in (8, 1 << 31, 8 | abi.PREEMPT_DEVICE):          # unknown bits, and they leave the mode as it was
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))
        res, _ = e.preempt(m.pres, ext=m.ext)
        assert_records_equal(res, m.res, "results after refused mode words")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream")
        res, _ = e.preempt(m.pres, ext=m.ext)                      # a refused call leaves the context usable
        assert_records_equal(res, m.res, "results after a refused stream")
        bad = m.ext.copy()
        bad["pts_n"][0] = 1
        bad["pts_skew"][0, 0] = 1
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=bad))     # a spread field
        res, _ = e.preempt(m.pres, ext=m.ext)
        assert_records_equal(res, m.res, "results after a refused record")
        e.preempt_set_mode(flags=0)                                # set_mode(0) restores the refusal
        for call in calls:
            expect(abi.E_INVAL, lambda: call(e))
    with loaded(Engine, m) as e:                                   # DEVICE | NUMA_FROZEN is accepted without NUMA
        e.preempt_set_mode(numa_frozen=True, device=True)
        res, _ = e.preempt(m.pres, ext=m.ext)
    assert_records_equal(res, m.res, "results under both flags")


def test_mode_on_other_profiles(Engine):
    p = M.case("wave")                                             # Fit + LoadAware: no DeviceShare
    with Engine(p.prof, device=0) as e:
        for bits in (abi.PREEMPT_DEVICE, abi.PREEMPT_DEVICE | abi.PREEMPT_RESV):
            expect(abi.E_INVAL, lambda: e.preempt_set_mode(flags=bits))
        e.load_snapshot(p.table)
        e.preempt_load_pods(p.assigned, p.pdb_allowed)
        res, _ = e.preempt(p.pres)                                 # the mode stayed 0
        expect(abi.E_INVAL, lambda: e.preempt(p.pres, ext=abi.pod_ext_array(len(p.pres))))
    assert_records_equal(res, p.res, "the plain profile after refused words")
    m = D.case("wave")
    rprof = with_deviceshare(shipped_profile(reservation=True))    # Reservation + DeviceShare: the follow-up
    with Engine(rprof, device=0) as e:
        e.preempt_set_mode(device=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="KOORDHIP_PREEMPT_RESV")
        e.preempt_set_mode(device=True, resv=True)
        expect(abi.E_INVAL, lambda: e.preempt_node_verdicts(m.pres[0]), match="follow-up")
    sprof = with_interpod_affinity(with_topology_spread(m.prof))   # state of their own
    with Engine(sprof, device=0) as e:
        e.preempt_set_mode(device=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        expect(abi.E_INVAL, lambda: e.preempt(m.pres, ext=m.ext), match="PodTopologySpread")


# ------------------------------------------------------------ 6. refused tables
def test_refused_tables_leave_the_old_one(Engine):
    m = D.case("wave")
    assert m.table.dev_slots == 8
    j = int(np.flatnonzero(m.ax["dev_slots"][:, D.G])[0])
    with loaded(Engine, m) as e:
        for field, index, value in (("dev_per", (j, D.G, 0), 1 << 45), ("xreq", (j, 0), 1 << 45), ("dev_per", (j, D.G, 1), -1),
                                    ("xmask", (j,), 1 << abi.NXRES)):
            ax = m.ax.copy()
            ax[field][index] = value
            expect(abi.E_INVAL, lambda: e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=ax))
            res, _ = e.preempt(m.pres, ext=m.ext)
            assert_records_equal(res, m.res, f"results after a refused table ({field})")
    t = m.table.copy()                                             # four device slots: a bit at slot 4 is past them
    for c in ("dev_minor", "dev_total", "dev_used"):
        t.cols[c] = np.ascontiguousarray(t[c][:, :, :4])
    t.dev_slots = 4
    ax = m.ax.copy()
    ax["dev_slots"][:] &= 15
    want = D.dry_run(m.base_cfg, t, m.assigned, m.pdb_allowed, m.pres, m.ext, ax)
    with Engine(m.prof, device=0) as e:
        e.preempt_set_mode(device=True)
        e.load_snapshot(t)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=ax)
        bad = ax.copy()
        bad["dev_slots"][j, D.G] = 1 << 4
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=bad), match="dev_slots")
        res, _ = e.preempt(m.pres, ext=m.ext)
    assert_records_equal(res, want[0], "results after a slot bit past dev_slots")
    p = M.case("wave")                                             # no device columns at all
    with Engine(p.prof, device=0) as e:
        e.load_snapshot(p.table)
        e.preempt_load_pods(p.assigned, p.pdb_allowed)
        held = np.zeros(len(p.assigned), abi.ASSIGNED_EXT_DTYPE)
        held["dev_slots"][0, D.G] = 1
        expect(abi.E_INVAL, lambda: e.preempt_load_pods(p.assigned, p.pdb_allowed, ext=held), match="no device columns")
        res, _ = e.preempt(p.pres)
    assert_records_equal(res, p.res, "the plain table after a refused one")
