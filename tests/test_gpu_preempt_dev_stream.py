"""The sequential preemption dry run under DeviceShare
(koordhip_preempt_stream_ext in the KOORDHIP_PREEMPT_DEVICE mode) on a real
MI355X against the plain-Python model (preempt_dev_stream_model.py), byte for
byte: the result records, the victims and the three stats counters; the
model's second form on the device (koordhip_preempt_ext on reloaded, rebuilt
tables); the lack of side effects and the refusals."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import (shipped_profile, with_deviceshare, with_interpod_affinity, with_topology_spread)

import preempt_dev_model as D
import preempt_dev_stream_model as T
import preempt_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def loaded(Engine, m, device=True):
    e = Engine(m.prof, device=0)
    e.preempt_set_mode(numa_frozen=m.numa, device=device)
    e.load_snapshot(m.table)
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


# ------------------------------------------- 1. records, victims, stats: the model
@pytest.mark.parametrize("name", T.ALL_CASES)
def test_stream_against_the_model(Engine, name):
    """One lane; a wave; a second node block and a second preemptor tile with
    eight device slots and a list past 64 pods; the frozen NUMA plane; the
    hand-worked cases.  max_victims exact, 0 and 1."""
    m = T.case(name)
    exact = max(1, int(m.res["best"]["n_victims"].max()))
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(m.pres, max_victims=exact, ext=m.ext)
        res0, vic0, st0 = e.preempt_stream(m.pres, max_victims=0, ext=m.ext)
        res1, vic1, st1 = e.preempt_stream(m.pres, max_victims=1, ext=m.ext)
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


def test_ext_null_is_zeroed_records(Engine):
    m = T.case("tiles")
    zero = abi.pod_ext_array(len(m.pres))
    with loaded(Engine, m) as e:
        res_n, vic_n, st_n = e.preempt_stream(m.pres, max_victims=3, ext=Engine.EXT_NULL)
        res_z, vic_z, st_z = e.preempt_stream(m.pres, max_victims=3, ext=zero)
    assert_records_equal(res_n, res_z, "results")
    assert_records_equal(vic_n, vic_z, "victims")
    assert st_n == st_z
    want = T.stream(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres[:6], zero[:6], m.ax)
    assert_records_equal(res_n[:6], want[0], "results against the model without requests")


def test_batch_of_non_device_preemptors(Engine):
    """No preemptor of the call has KOORDHIP_PODX_DEVICE: the scalars-only walk (DEV = 1) on a table whose pods hold
    scalars, some preemptors with a scalar request so that the second table is read."""
    m = T.case("tiles")
    keep = np.flatnonzero((m.ext["flags"] & abi.PODX_DEVICE) == 0)
    assert len(keep) >= 2
    ext = m.ext[keep].copy()
    k = D.XRES_INDEX[D.NVIDIA_GPU]
    ext["xreq"][::2, k], ext["xmask"][::2] = 1, 1 << k
    pres = m.pres[keep]
    want_res, want_chosen, want_stats, _ = T.stream(m.base_cfg, m.table, m.assigned, m.pdb_allowed, pres, ext, m.ax)
    with loaded(Engine, m) as e:
        res, vic, st = e.preempt_stream(pres, max_victims=2, ext=ext)
    assert_records_equal(res, want_res, "results")
    assert_records_equal(vic, M.victims_array(want_chosen, 2), "victims")
    assert st == want_stats


def test_one_preemptor_is_preempt_ext(Engine):
    m = T.case("wave")
    with loaded(Engine, m) as e:
        for p in range(len(m.pres)):
            res, vic, _ = e.preempt_stream(m.pres[p:p + 1], max_victims=4, ext=m.ext[p:p + 1])
            res1, vic1 = e.preempt(m.pres[p:p + 1], max_victims=4, ext=m.ext[p:p + 1])
            assert_records_equal(res, res1, f"preemptor {p}: result")
            assert_records_equal(vic, vic1, f"preemptor {p}: victims")


# ------------------------------------------- 2. the model's second form on the device
def test_rebuilt_tables_on_the_device(Engine):
    """For the first four preemptors of `wave`: koordhip_preempt_ext of the one preemptor on a context loaded with
    the table rebuilt without V_0..V_{k-1} and with the nominated pods is the stream's record."""
    m = T.case("wave")
    with loaded(Engine, m) as e:
        res, vic, _ = e.preempt_stream(m.pres, max_victims=8, ext=m.ext)
    nodes = [int(x) for x in res["node"]]
    chosen = [[int(j) for j in v if j >= 0] for v in vic]
    assert max(len(c) for c in chosen) < 8
    assert sum(1 for x in nodes[:3] if x >= 0) >= 1, "an earlier preemptor found a node"
    for k in range(4):
        t, a_k, ax_k, allowed, pre, keep = T.rebuilt_inputs(m.table, m.assigned, m.pdb_allowed, m.pres, m.ext, m.ax, k,
                                                           chosen, nodes)
        with Engine(m.prof, device=0) as e:
            e.preempt_set_mode(device=True)
            e.load_snapshot(t)
            e.preempt_load_pods(a_k, allowed, ext=ax_k)
            r, v = e.preempt(pre, max_victims=8, ext=m.ext[k:k + 1])
        assert_records_equal(r[0], res[k], f"preemptor {k}: result on the rebuilt table")
        assert [int(keep[j]) for j in v[0] if j >= 0] == chosen[k], f"preemptor {k}: victims on the rebuilt table"


# ------------------------------------------------------- 3. no side effects
def test_stream_changes_no_state(Engine):
    m = T.case("tiles")
    d = D.case("tiles")
    stream = synth.make_pods(synth.StreamSpec(150, be_frac=0.3, seed=11), m.prof)
    sext = synth.make_device_ext(150, synth.DevStreamSpec(frac=0.3))
    with loaded(Engine, m) as e:
        n0, d0 = e.read_nodes(), e.read_devices()
        e.preempt_stream(m.pres, max_victims=4, ext=m.ext)
        n1, d1 = e.read_nodes(), e.read_devices()
        for k in n0:
            assert n0[k].tobytes() == n1[k].tobytes(), k
        for k in d0:
            assert d0[k].tobytes() == d1[k].tobytes(), k
        res, vic = e.preempt(m.pres, max_victims=4, ext=m.ext)       # the loaded table and its second table are as they were
        after = e.place_stream_ext(stream, sext)
    assert_records_equal(res, d.res, "the independent batch after the stream")
    assert_records_equal(vic, M.victims_array(d.chosen, 4), "its victims")
    assert np.array_equal(after, oracle.Oracle(m.cfg, m.table).place_stream_ext(stream, sext))


# ------------------------------------------------------------ 4. the refusals
def test_refused_outside_the_mode(Engine):
    m = T.case("wave")
    with loaded(Engine, m, device=False) as e:
        for ext in (m.ext, Engine.EXT_NULL):                       # with records or with NULL
            expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=ext), match="koordhip_preempt_stream_ext")
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream_ext")   # the plain call names it
        e.preempt_set_mode(device=True)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres), match="koordhip_preempt_stream_ext")
        res, _, st = e.preempt_stream(m.pres, ext=m.ext)            # refused calls leave the context answering
    assert_records_equal(res, m.res, "results after refused calls")
    assert st == m.stats
    p = M.case("wave")                                             # Fit + LoadAware: no DeviceShare, no DEVICE mode
    with Engine(p.prof, device=0) as e:
        e.load_snapshot(p.table)
        e.preempt_load_pods(p.assigned, p.pdb_allowed)
        expect(abi.E_INVAL, lambda: e.preempt_stream(p.pres, ext=Engine.EXT_NULL), match="koordhip_preempt_stream_ext")
        res, _ = e.preempt(p.pres)
    assert_records_equal(res, p.res, "the plain profile after a refused call")


def test_refused_records_and_preemptors(Engine):
    m = T.case("numa")
    with loaded(Engine, m) as e:
        bad = m.ext.copy()
        bad["pts_n"][0] = 1
        bad["pts_skew"][0, 0] = 1
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=bad))            # a spread field
        bad = m.ext.copy()
        bad["xmask"][1] |= 1
        bad["xreq"][1, 0] = 1 << 45
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=bad), match="xreq")
        for flag in (abi.POD_RESERVE, abi.POD_RESV_OPERATING, abi.POD_NUMA_ERROR):
            pres = m.pres.copy()
            pres["pod"]["flags"][1] |= flag
            expect(abi.E_INVAL, lambda: e.preempt_stream(pres, ext=m.ext))
        res, vic, st = e.preempt_stream(m.pres, ext=m.ext)
    assert_records_equal(res, m.res, "results after refused calls")
    assert st == m.stats


def test_refused_profiles(Engine):
    m = T.case("wave")
    rprof = with_deviceshare(shipped_profile(reservation=True))    # Reservation state beside the flag: the follow-up
    with Engine(rprof, device=0) as e:
        e.preempt_set_mode(device=True, resv=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=m.ext), match="follow-up")
    sprof = with_interpod_affinity(with_topology_spread(m.prof))   # state of their own
    with Engine(sprof, device=0) as e:
        e.preempt_set_mode(device=True)
        e.load_snapshot(m.table)
        e.preempt_load_pods(m.assigned, m.pdb_allowed, ext=m.ax)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=m.ext), match="PodTopologySpread")


def test_refused_with_a_communicator(Engine):
    m = T.case("wave")
    with loaded(Engine, m) as e:
        e.comm_init(Engine.comm_unique_id(), 1, 0)
        expect(abi.E_INVAL, lambda: e.preempt_stream(m.pres, ext=m.ext), match="communicator")
