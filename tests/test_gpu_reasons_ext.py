"""koordhip_diagnose_reasons_ext / koordhip_node_reasons_ext on a real MI355X
against the CPU model (reasons_ext_model.py), bit for bit: records and node
masks of every case and of the directed table, the pod tiling, the state after a
stream, the ties to koordhip_node_status_ext and koordhip_diagnose_ext, byte
equality with koordhip_diagnose_reasons where both answer, the lack of side
effects and the validation errors."""
import numpy as np
import pytest

import diag_ext_model as X
import diag_model as M
import reasons_ext_model as XM
from koordinator_amd import abi, diagnosis, synth
from koordinator_amd.config import shipped_profile

pytestmark = pytest.mark.gpu

BIG = "full-1003x70"
OF = abi.REASONS_OF_BIT_EXT


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def assert_records_equal(got, want, loose=0):
    """`loose`: reason groups without a model (XM.masks) -- their slots, and what depends on which plugin
    failed first, are not compared."""
    fields = ("feasible", "unresolvable", "first", "any") if not loose else ("any",)
    keep = np.array([not (loose >> r) & 1 for r in range(abi.REASON_SLOTS)])
    for f in fields:
        g, w = (got[f][:, keep], want[f][:, keep]) if f == "any" else (got[f], want[f])
        if not np.array_equal(g, w):
            bad = int(np.flatnonzero((g != w).reshape(len(got), -1).any(axis=1))[0])
            raise AssertionError(f"{f} differs first at pod {bad}: got {got[bad]} want {want[bad]}")


def ext_of(x, j):
    return None if x.ext is None else x.ext[j]


# --------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", XM.CASES)
def test_reasons_ext_is_the_model(Engine, name):
    m = XM.case(name)
    x = m.x
    n = x.table.n
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        rec = e.diagnose_reasons_ext(x.pods, x.ext)
        masks = np.stack([e.node_reasons_ext(x.pods[j], ext_of(x, j)) for j in range(len(x.pods))])
        status = np.stack([e.node_status_ext(x.pods[j], ext_of(x, j)) for j in range(len(x.pods))])
        diag = e.diagnose_ext(x.pods, x.ext)
    assert masks.dtype == np.uint32
    # the node masks: the model's, and the status they stand for is node_status_ext's (every group)
    assert np.array_equal(masks & ~np.uint32(m.loose), m.mask)
    assert np.array_equal(abi.reasons_status_ext(masks), status.astype(np.uint32))
    assert np.array_equal(status, x.status)
    # the records: the histogram of the node masks, and the model's
    assert_records_equal(rec, XM.records(masks))
    assert_records_equal(rec, m.rec, m.loose)
    first = abi.first_reasons_ext(masks)
    assert (rec["feasible"] + (first != 0).sum(axis=1) == n).all()
    # per-group ties to diagnose_ext's record
    assert np.array_equal(rec["feasible"], diag["feasible"])
    fit = OF[abi.ST_FIT_FAIL] | OF[abi.ST_XFIT_FAIL]
    for b, group in OF.items():
        slots = [r for r in range(abi.REASON_SLOTS) if (group >> r) & 1]
        k = b.bit_length() - 1
        if b in (abi.ST_FIT_FAIL, abi.ST_XFIT_FAIL):        # once per failing resource here, once per node there
            assert (rec["any"][:, slots].max(axis=1) <= diag["any"][:, k]).all()
            assert (diag["any"][:, k] <= rec["any"][:, slots].sum(axis=1)).all()
        else:
            assert np.array_equal(rec["any"][:, slots].sum(axis=1), diag["any"][:, k]), b
            assert np.array_equal(rec["first"][:, slots].sum(axis=1), diag["first"][:, k]), b
    kf, kx = abi.ST_FIT_FAIL.bit_length() - 1, abi.ST_XFIT_FAIL.bit_length() - 1
    assert np.array_equal(((first & np.uint32(fit)) != 0).sum(axis=1), diag["first"][:, kf] + diag["first"][:, kx])


def test_directed_table(Engine):
    """The hand-written masks, through the engine."""
    x = XM.directed()
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        rec = e.diagnose_reasons_ext(x.pods, x.ext)
        masks = np.stack([e.node_reasons_ext(x.pods[j], x.ext[j]) for j in range(len(x.pods))])
    for p, want in XM.D_WANT.items():
        assert [hex(int(v)) for v in masks[p]] == [hex(v) for v in want], p
    for p, helps in XM.D_PREEMPTION_HELPS.items():
        assert diagnosis.preemption_might_help(rec[p], XM.D_N) == helps, p
    msg = diagnosis.fit_error_message(rec[0], XM.D_N)
    parts = msg[len(f"0/{XM.D_N} nodes are available: "):-1].split(", ")
    assert "2 " + diagnosis.reason_text(abi.REASON_FIT_X0 + 2) in parts and "3 Insufficient cpu" not in parts, msg
    assert "2 Insufficient cpu" in parts, msg


# ----------------------------------------------------------- 2. pod tiling
def test_records_do_not_depend_on_the_pod_tiling(Engine):
    m = XM.case(BIG)
    x = m.x
    T = abi.DIAG_EXT_POD_TILE
    assert 1 < T and T + 1 < len(x.pods)
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        whole = e.diagnose_reasons_ext(x.pods, x.ext)
        assert_records_equal(whole, m.rec)
        for k in (1, T, T + 1):
            assert e.diagnose_reasons_ext(x.pods[:k], x.ext[:k]).tobytes() == whole[:k].tobytes(), k


# -------------------------------------------------------- 3. current state
def test_answers_on_the_current_state(Engine):
    """Sums or tables kept from an earlier call would give the pre-stream records."""
    m = XM.case(BIG)
    x = m.x
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        before = e.diagnose_reasons_ext(x.pods, x.ext)
        out = e.place_stream_ext(x.pods, x.ext)
        after = e.diagnose_reasons_ext(x.pods, x.ext)
        mid = len(x.pods) // 2
        row = e.node_reasons_ext(x.pods[mid], x.ext[mid])
    assert np.array_equal(out, x.out)
    assert_records_equal(before, m.rec)
    assert_records_equal(after, m.rec_after)
    assert int((after != before).sum()) >= 10
    assert np.array_equal(row, m.mask_after[mid])


# ------------------------------------------------------- 4. no side effects
def state_bytes(e):
    parts = {}
    for name, d in (("nodes", e.read_nodes()), ("numa", e.read_numa()), ("devices", e.read_devices())):
        for k, v in d.items():
            parts[f"{name}.{k}"] = v.tobytes()
    parts["pts"] = e.read_pts().tobytes()
    parts["ipa"] = e.read_ipa().tobytes()
    return parts


def test_changes_no_state(Engine):
    x = XM.case(BIG).x
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        s0 = state_bytes(e)
        e.diagnose_reasons_ext(x.pods, x.ext)
        e.node_reasons_ext(x.pods[-1], x.ext[-1])
        s1 = state_bytes(e)
        out = e.place_stream_ext(x.pods, x.ext)
    assert s0.keys() == s1.keys()
    for k in s0:
        assert s0[k] == s1[k], k
    assert np.array_equal(out, x.out)


def test_fetch_diagnosis_still_works_afterwards(Engine):
    m = M.case("B")
    with Engine(m.prof, device=0) as e:
        e.load_snapshot(m.table)
        out = e.place_stream(m.pods)
        cur = e.diagnose_reasons_ext(m.pods[m.unplaced])
        want = e.diagnose_reasons(m.pods[m.unplaced])
        got = e.fetch_diagnosis(len(m.pods))
    assert np.array_equal(out, m.out)
    assert cur.tobytes() == want.tobytes()
    for f in ("feasible", "any", "first"):
        assert np.array_equal(got[f], m.rec[f]), f


# ---------------------------------------------------------- 5. equivalence
def test_equals_diagnose_reasons_on_a_plain_profile(Engine):
    x = X.plain()
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        assert e.diagnose_reasons_ext(x.pods, None).tobytes() == e.diagnose_reasons(x.pods).tobytes()
        assert np.array_equal(e.node_reasons_ext(x.pods[3]), e.node_reasons(x.pods[3]))


def test_ext_none_on_a_sequential_cycle_profile(Engine):
    """No pod carries a record: the ext plugins have nothing to fail, the base plugins answer as with empty records."""
    x = X.full(63, 7)
    empty = abi.pod_ext_array(len(x.pods))
    with Engine(x.prof, device=0) as e:
        e.load_snapshot(x.table)
        got = e.diagnose_reasons_ext(x.pods, None)
        assert got.tobytes() == e.diagnose_reasons_ext(x.pods, empty).tobytes()
        assert np.array_equal(e.node_reasons_ext(x.pods[0]), e.node_reasons_ext(x.pods[0], empty[0]))
    assert not got["any"][:, abi.REASON_COUNT:].any()


# -------------------------------------------------------------- 6. envelope
def raises(code, call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == code


def test_envelope(Engine):
    m = XM.case("resv")
    x = m.x
    with Engine(x.prof, device=0) as e:
        raises(abi.E_STATE, lambda: e.diagnose_reasons_ext(x.pods, x.ext))              # no snapshot
        raises(abi.E_STATE, lambda: e.node_reasons_ext(x.pods[0], x.ext[0]))
        e.load_snapshot(x.table)
        assert len(e.diagnose_reasons_ext(x.pods[:0], x.ext[:0])) == 0                  # n_pods = 0
        rp = x.pods[:2].copy()
        rp["flags"][1] |= abi.POD_RESERVE
        rp["resv_match"][1] = 0
        raises(abi.E_INVAL, lambda: e.diagnose_reasons_ext(rp, x.ext[:2]))              # a reserve pod
        raises(abi.E_INVAL, lambda: e.node_reasons_ext(rp[1], x.ext[1]))
        bad = x.ext[:1].copy()
        bad["xmask"][0] = 1 << abi.NXRES
        raises(abi.E_INVAL, lambda: e.diagnose_reasons_ext(x.pods[:1], bad))            # a bad ext record
        assert_records_equal(e.diagnose_reasons_ext(x.pods, x.ext), m.rec, m.loose)     # the errors left nothing behind
    prof = shipped_profile()
    table = synth.make_cluster(synth.ClusterSpec(64), prof)
    pods = synth.make_pods(synth.StreamSpec(4), prof)
    ext = synth.make_device_ext(4, synth.DevStreamSpec(frac=1.0))
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        raises(abi.E_INVAL, lambda: e.diagnose_reasons_ext(pods, ext))                  # a device request, no DeviceShare
        raises(abi.E_INVAL, lambda: e.node_reasons_ext(pods[0], ext[0]))
        assert e.diagnose_reasons_ext(pods, None).tobytes() == e.diagnose_reasons(pods).tobytes()
