"""koordhip_diagnose_ext / koordhip_node_status_ext on a real MI355X against the
CPU oracle, bit for bit (diag_ext_model.py): the records of every
sequential-cycle case, their independence of the kernel's pod tiling, one
pod's status words, the current state after a stream, the lack of side
effects, the equivalence with koordhip_diagnose where both answer, and the
validation errors."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config

import diag_ext_model as X
import diag_model as M

pytestmark = pytest.mark.gpu

BIG = X.FULL_SHAPES[-1]


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def assert_records_equal(got, want):
    for f in ("feasible", "any", "first"):
        if not np.array_equal(got[f], want[f]):
            bad = int(np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0])
            raise AssertionError(f"{f} differs first at pod {bad}: got {got[bad]} want {want[bad]}")
    assert not got["reserved"].any()


# --------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", sorted(X.CASES))
def test_diagnose_ext_equals_the_model(Engine, case):
    m = X.CASES[case]()
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        got = e.diagnose_ext(m.pods, m.ext)
    assert_records_equal(got, m.rec)
    assert (got["feasible"] + got["first"].sum(axis=1) == m.table.n).all()


# ----------------------------------------------------------- 2. pod tiling
def test_records_do_not_depend_on_the_pod_tiling(Engine):
    m = X.full(*BIG)
    T = abi.DIAG_EXT_POD_TILE
    assert 1 < T and T + 1 < len(m.pods)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        whole = e.diagnose_ext(m.pods, m.ext)
        assert_records_equal(whole, m.rec)
        for k in (1, T, T + 1):
            assert e.diagnose_ext(m.pods[:k], m.ext[:k]).tobytes() == whole[:k].tobytes(), k


# ------------------------------------------------------ 3. node_status_ext
@pytest.mark.parametrize("case", ["full", "resv"])
def test_node_status_ext(Engine, case):
    m = X.full(*BIG) if case == "full" else X.resv()
    picks = [0, len(m.pods) // 2, len(m.pods) - 1]
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        got = {j: e.node_status_ext(m.pods[j], m.ext[j]) for j in picks}
    for j in picks:
        assert got[j].dtype == np.uint16
        assert np.array_equal(got[j], m.status[j]), j


# -------------------------------------------------------- 4. current state
def test_diagnose_ext_answers_on_the_current_state(Engine):
    """Sums or tables kept from an earlier call would give the pre-stream records."""
    m = X.full(*BIG)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        before = e.diagnose_ext(m.pods, m.ext)
        out = e.place_stream_ext(m.pods, m.ext)
        after = e.diagnose_ext(m.pods, m.ext)
        mid = len(m.pods) // 2
        st = e.node_status_ext(m.pods[mid], m.ext[mid])
    assert np.array_equal(out, m.out)
    assert_records_equal(before, m.rec)
    assert_records_equal(after, m.rec_after)
    assert int((after != before).sum()) >= 10
    assert np.array_equal(st, m.status_after[mid])


# ------------------------------------------------------- 5. no side effects
def state_bytes(e):
    parts = {}
    for name, d in (("nodes", e.read_nodes()), ("numa", e.read_numa()), ("devices", e.read_devices())):
        for k, v in d.items():
            parts[f"{name}.{k}"] = v.tobytes()
    parts["pts"] = e.read_pts().tobytes()
    parts["ipa"] = e.read_ipa().tobytes()
    return parts


def test_diagnose_ext_changes_no_state(Engine):
    m = X.full(*BIG)
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        s0 = state_bytes(e)
        e.diagnose_ext(m.pods, m.ext)
        e.node_status_ext(m.pods[-1], m.ext[-1])
        s1 = state_bytes(e)
        out = e.place_stream_ext(m.pods, m.ext)
    assert s0.keys() == s1.keys()
    for k in s0:
        assert s0[k] == s1[k], k
    assert np.array_equal(out, m.out)


def test_fetch_diagnosis_still_works_after_diagnose_ext(Engine):
    m = M.case("B")
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        out = e.place_stream(m.pods)
        cur = e.diagnose_ext(m.pods[m.unplaced])
        got = e.fetch_diagnosis(len(m.pods))
    assert np.array_equal(out, m.out)
    assert_records_equal(cur, m.final_rec[m.unplaced])
    assert_records_equal(got, m.rec)


# ---------------------------------------------------------- 6. equivalence
def test_equals_diagnose_on_a_plain_profile(Engine):
    m = X.plain()
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        assert e.diagnose_ext(m.pods, None).tobytes() == e.diagnose(m.pods).tobytes()


def test_equals_diagnose_on_a_reservation_snapshot(Engine):
    prof = shipped_profile(numa=True, reservation=True)
    table = synth.make_cluster(synth.ClusterSpec(400), prof)
    synth.add_numa(table, synth.NumaSpec(), prof)
    synth.add_reservations(table, synth.ResvSpec())
    pods = synth.make_pods(synth.StreamSpec(40, be_frac=0.3, cpuset_frac=0.3, resv_match_frac=0.3), prof)
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        got = e.diagnose_ext(pods, None)
        assert got.tobytes() == e.diagnose(pods).tobytes()
    ref = oracle.Oracle(to_c_config(prof), table).eval(pods, status=True, scores=False)["status"]
    assert_records_equal(got, M.records(ref))


# -------------------------------------------------------------- 7. envelope
def raises(code, call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == code


def test_envelope(Engine):
    m = X.resv()
    with Engine(m.prof, device=0) as e:
        raises(abi.E_STATE, lambda: e.diagnose_ext(m.pods, m.ext))                    # no snapshot
        e.load_snapshot(m.table)
        assert len(e.diagnose_ext(m.pods[:0], m.ext[:0])) == 0                        # n_pods = 0
        rp = m.pods[:2].copy()
        rp["flags"][1] |= abi.POD_RESERVE
        rp["resv_match"][1] = 0
        raises(abi.E_INVAL, lambda: e.diagnose_ext(rp, m.ext[:2]))                    # a reserve pod
        raises(abi.E_INVAL, lambda: e.node_status_ext(rp[1], m.ext[1]))
        assert_records_equal(e.diagnose_ext(m.pods, m.ext), m.rec)                    # the errors left nothing behind
    prof = shipped_profile()
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    pods = synth.make_pods(synth.StreamSpec(4), prof)
    ext = synth.make_device_ext(4, synth.DevStreamSpec(frac=1.0))
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        raises(abi.E_INVAL, lambda: e.diagnose_ext(pods, ext))                        # a device request, no DeviceShare
        raises(abi.E_INVAL, lambda: e.node_status_ext(pods[0], ext[0]))
        assert e.diagnose_ext(pods, None).tobytes() == e.diagnose(pods).tobytes()
