"""The model of the preemption dry run under DeviceShare (preempt_dev_model.py)
on the CPU: the reference's own tables through it, its agreement with the
oracle where nothing is removed, the literal maps against the linear form the
kernel keeps, the hand-worked cases, the coverage of the generated ones and the
host records."""
import json
import os

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, deviceshare, k8s, preemption
from koordinator_amd.marshal import MarshalError

import preempt_dev_model as D
import preempt_model as M

AX = abi.ASSIGNED_EXT_DTYPE        # (the whole file is about the DEVICE mode's records)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "preempt_deviceshare.json")
TYPES = {"gpu": abi.DEV_GPU, "rdma": abi.DEV_RDMA, "fpga": abi.DEV_FPGA}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _maps(d):
    return {TYPES[t]: {int(m): list(v) for m, v in devs.items()} for t, devs in d.items()}


# ------------------------------------------------------ the reference's tables
def test_prefilter_extension_rows():
    for row in golden()["prefilter_extensions"]:
        state = {}
        alloc = _maps(row["pod_allocated"])
        D.remove_pod(state, alloc)
        assert state == _maps(row["after_remove"]), row["source"]
        D.add_pod(state, alloc)
        assert state == _maps(row["after_add"]), row["source"]


def test_filter_rows():
    for row in golden()["filter"]:
        total, used = _maps(row["total"]), _maps(row.get("used", {}))
        node = {}
        for t, devs in total.items():
            node[t] = {"minors": sorted(devs), "total": devs,
                       "used": {m: used.get(t, {}).get(m, [0] * abi.DEV_RES) for m in devs}}
        req = np.zeros((abi.DEV_TYPES, abi.DEV_RES), np.int64)
        req[abi.DEV_GPU] = -1
        for t, q in row["request"].items():
            req[TYPES[t]] = q
        pre = _maps(row["preemptible"])
        assert D.device_filter(req, node, pre) == row["passes"], row["source"]
        # the linear form on the same row (minors renumbered as slots)
        slots = {t: {m: s for s, m in enumerate(sorted(devs))} for t, devs in total.items()}
        lin = {t: {"minors": list(range(len(devs))), "total": {slots[t][m]: v for m, v in devs.items()},
                   "used": {slots[t][m]: node[t]["used"][m] for m in devs}} for t, devs in total.items()}
        pd = np.zeros((abi.DEV_TYPES, abi.DEV_SLOTS, abi.DEV_RES), np.int64)
        for t, devs in pre.items():
            for mnr, v in devs.items():
                pd[t, slots[t][mnr]] = v
        assert D.linear_filter(req, lin, pd) == row["passes"], row["source"]


# ------------------------------------------- nothing removed: the oracle's bits
def test_start_rows_agree_with_the_oracle():
    m = D.case("wave")
    pods = np.ascontiguousarray(m.pres["pod"])
    st = oracle.Oracle(m.cfg, m.table).eval_ext(pods, m.ext, status=True, scores=False)["status"]
    nodes = [D.node_devices(m.table, i) for i in range(m.table.n)]
    seen = set()
    for p in range(len(m.pres)):
        x = m.ext[p]
        for i in range(m.table.n):
            dev = not (int(x["flags"]) & abi.PODX_DEVICE) or D.device_filter(x["dev_req"], nodes[i], {})
            xf = D.xfit(x, m.table["xalloc"][i], m.table["xrequested"][i])
            assert dev == (not (int(st[p, i]) & abi.ST_DEVICE_FAIL)), (p, i)
            assert xf == (not (int(st[p, i]) & abi.ST_XFIT_FAIL)), (p, i)
            seen.add((dev, xf))
    assert len(seen) == 4


# ------------------------------------------------- literal maps = linear form
@pytest.mark.parametrize("name", D.ALL_CASES)
def test_no_clamp_ever_triggers(name):
    """DevRule asserts the equality after every move and in every fit test; the
    clamps and the missing-minor exit of subtract are counted and never taken."""
    m = D.case(name)
    assert "subtract_clamped" not in m.branches and "subtract_missing_minor" not in m.branches
    assert (m.res["count"].sum(axis=1) == m.table.n).all()


# ------------------------------------------------------------- directed cases
@pytest.mark.parametrize("name", D.DIRECTED)
def test_directed_cases(name):
    m = D.case(name)
    got = [(int(m.verdicts[0][i]["status"]), m.victims[0][i]) for i in range(m.table.n)]
    assert got == D.EXPECTED[name]


def test_directed_cases_depend_on_the_freed_devices():
    """Without the second table (nothing is freed) `freed` has no candidate and `scalar` none either."""
    for name in ("freed", "share", "scalar"):
        m = D.case(name)
        res = D.dry_run(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.ext, None)[0]
        assert int(res["node"][0]) == -1 and int(res["count"][0][abi.PREEMPT_UNFIT]) == 1, name


# ------------------------------------------------------------------- coverage
def test_generated_cases_cover_the_branches():
    m = D.case("tiles")
    b = m.branches
    for need in ("freed_decides",          # a pair decided by freed devices
                 "device_unfit",           # UNFIT through devices alone
                 "device_victim",          # a victim kept for its device
                 "xfit_victim",            # an XFIT-decided victim
                 "non_device_preemptor", "free_merged", "free_plain"):
        assert b.get(need, 0) > 0, (need, b)
    # a list past 64 pods with a device pod beyond position 64
    lists = M.node_lists(m.assigned, m.table.n)
    long = lists[M.FULL_NODE]
    assert len(long) > 64 and any(m.ax["dev_slots"][j].any() for j in long[64:])
    # a node with all 8 slots of a type
    assert m.table.dev_slots == 8 and (m.table["dev_minor"][:, abi.DEV_GPU] >= 0).all(axis=1).any()
    # a second node tile and a second preemptor tile
    assert m.table.n > 256 and len(m.pres) > 32
    assert (m.res["node"] >= 0).any() and (m.res["best"]["n_victims"] > 0).any()


# ----------------------------------------------------- the tie to the plain model
def test_empty_records_are_the_plain_dry_run():
    p = M.case("tiles")
    t = p.table.copy()
    t.enable_ext(dev_slots=0)
    res, ver, chosen, _, _ = D.dry_run(p.cfg, t, p.assigned, p.pdb_allowed, p.pres, None, None)
    assert res.tobytes() == p.res.tobytes()
    assert ver.tobytes() == p.verdicts.tobytes()
    assert chosen == p.chosen


# --------------------------------------------------------------- host records
def _pod(name, node, annotation=None, requests=None):
    return k8s.Pod(name=name, node_name=node, annotations={deviceshare.ANNOTATION_DEVICE_ALLOCATED: annotation} if annotation else {},
                   containers=[k8s.Container(requests={n: k8s.Quantity(v) for n, v in (requests or {}).items()})])


def test_assigned_ext_records_round_trip():
    m = D.case("reprieve")
    t = m.table.copy()
    t["dev_minor"][0, abi.DEV_GPU, :2] = (3, 5)            # minors 3 and 5 in slots 0 and 1
    ann = json.dumps({"gpu": [{"minor": 5, "resources": {deviceshare.GPU_CORE: "100", deviceshare.GPU_MEMORY_RATIO: "100",
                                                         deviceshare.GPU_MEMORY: "16Gi"}},
                              {"minor": 9, "resources": {deviceshare.GPU_CORE: "100"}}]})   # 9: not on the node, dropped
    pods = [_pod("a", "n0", ann, {deviceshare.NVIDIA_GPU: "1"}), _pod("b", "elsewhere"), _pod("c", "n0")]
    rec = preemption.assigned_ext_records(pods, t, {"n0": 0})
    assert rec.dtype == AX and len(rec) == 2
    assert int(rec["dev_slots"][0, abi.DEV_GPU]) == 1 << 1
    assert [int(v) for v in rec["dev_per"][0, abi.DEV_GPU]] == [100, 100, 16 * D.GI]
    k = deviceshare.XRES_INDEX[deviceshare.NVIDIA_GPU]
    assert int(rec["xmask"][0]) == 1 << k and int(rec["xreq"][0, k]) == 1
    assert not rec[1].tobytes().strip(b"\0")
    # back to the annotation's minors
    assert deviceshare.slot_minors(t, 0, rec["dev_slots"][0]) == {"gpu": [5]}
    bad = json.dumps({"gpu": [{"minor": 3, "resources": {deviceshare.GPU_CORE: "50"}},
                              {"minor": 5, "resources": {deviceshare.GPU_CORE: "100"}}]})
    with pytest.raises(MarshalError, match="different amounts"):
        preemption.assigned_ext_records([_pod("d", "n0", bad)], t, {"n0": 0})
    x = preemption.preemptor_ext_records([_pod("p", "", None, {deviceshare.KOORD_GPU: "200"})])
    assert x.dtype == abi.POD_EXT_DTYPE and int(x["flags"][0]) & abi.PODX_DEVICE
    assert [int(v) for v in x["dev_req"][0, abi.DEV_GPU]] == [200, 200, -1]


def test_abi_is_additive():
    lib = abi.load_library()
    assert abi.KOORDHIP_ABI_VERSION == 15 and abi.PREEMPT_DEVICE == 4
    for name in ("koordhip_preempt_load_pods_ext", "koordhip_preempt_ext", "koordhip_preempt_node_verdicts_ext"):
        assert hasattr(lib, name) and name in abi.EXPORTED_SYMBOLS and name in abi.ADDITIVE_SYMBOLS
    assert AX.itemsize == 160 and abi.ASSIGNED_DTYPE.itemsize == 160
