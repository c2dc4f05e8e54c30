"""The model of the preemption dry run under DeviceShare beside Reservation
state (preempt_devresv_model.py) on the CPU: the hand-worked tables, the literal
maps against the linear form the kernel keeps, its agreement with the two
single-state models where one state is absent, the coverage of the case set, the
host records and the new constant.  (koordhip_preempt_set_mode's word rules
need the library on a device: test_gpu_preempt_devresv.py.)"""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from koordinator_amd import abi, deviceshare, k8s, preemption as pre, reservation as rsv
from koordinator_amd.config import shipped_profile, with_deviceshare

import preempt_dev_model as D
import preempt_devresv_model as B
import preempt_resv_model as V


# ------------------------------------------------------ 1. the hand-worked tables
@pytest.mark.parametrize("name", B.DIRECTED)
def test_directed_cases(name):
    m = B.case(name)
    assert len(B.EXPECTED[name]) == len(m.pres)
    for p, want in enumerate(B.EXPECTED[name]):
        got = [(int(m.verdicts[p]["status"][i]), m.victims[p][i]) for i in range(m.table.n)]
        assert got == want, (name, p)


def test_bound_victims_devices_are_not_freed():
    """bound_device's two nodes differ in the binding alone; under DeviceShare alone both are candidates."""
    m = B.case("bound_device")
    assert [int(s) for s in m.verdicts[0]["status"]] == [abi.PREEMPT_UNFIT, abi.PREEMPT_CANDIDATE]
    a = m.assigned.copy()
    a["flags"] &= ~np.uint32(abi.ASG_RESV_SLOT_MASK)
    unbound = B.dry_run(m.resv_cfg, m.table, a, m.pdb_allowed, m.pres, m.ext, m.ax, m.base_cfg)
    assert [int(s) for s in unbound[1][0]["status"]] == [abi.PREEMPT_CANDIDATE, abi.PREEMPT_CANDIDATE]


def test_the_scalars_in_the_maps_decide():
    """bound_scalar fails by fitsNode's scalar term alone; quirk_scalar's answer needs the scalar the preemptor
    does not request: a state over the five row resources (the records without their scalars) names a victim."""
    m = B.case("bound_scalar")
    assert m.branches.get("scalar_term_decides")
    q = B.case("quirk_scalar")
    assert q.victims[0][0] == []
    bare = q.ax.copy()
    bare["xmask"][:] = 0
    bare["xreq"][:] = 0
    t = q.table.copy()
    t["xrequested"][:] = 0
    five = B.dry_run(q.resv_cfg, t, q.assigned, q.pdb_allowed, q.pres, q.ext, bare, q.base_cfg)
    assert int(five[1][0]["status"][0]) == abi.PREEMPT_CANDIDATE and five[3][0][0] == [0]


# ---------------------------------------------- 2. literal form = linear form
@pytest.mark.parametrize("name", B.ALL_CASES)
def test_literal_maps_equal_the_linear_form(name):
    """DevResvRule asserts it after every move and in every fit test; the cases run through without one firing,
    and every verdict is one of a walk that ended."""
    m = B.case(name)
    assert m.verdicts.shape == (len(m.pres), m.table.n)
    assert (m.res["count"].sum(axis=1) == m.table.n).all()


def test_the_assertion_fires_on_a_wrong_linear_form():
    inp, ext, ax = B._DIRECTED["reprieve"]()

    class Wrong(B.DevResvRule):
        def moved(self, i, a, sign):
            self.pd[i, B.G, 1, 0] += 1 if V.bound_slot(a) >= 0 and sign < 0 else 0   # a bound pod's GPU, freed
            super().moved(i, a, sign)

    m = B.case("reprieve")
    rule = lambda *args: Wrong(*args, x=ext[0], ax=ax, assigned=inp.assigned, base_cfg=m.base_cfg)   # noqa: E731
    with pytest.raises(AssertionError):
        B.M.select_victims(m.resv_cfg, inp.table, inp.assigned, inp.pdb_allowed, inp.pres[0], None, rule)


# --------------------------------------- 3. one state absent: the other model
@pytest.mark.parametrize("name", ["wave", "numa", "share", "scalar"])
def test_without_reservation_columns_it_is_the_device_model(name):
    d = D.case(name)
    res, ver, chosen, _, _ = B.dry_run(d.base_cfg, d.table, d.assigned, d.pdb_allowed, d.pres, d.ext, d.ax, d.base_cfg)
    assert res.tobytes() == d.res.tobytes()
    assert ver.tobytes() == d.verdicts.tobytes()
    assert chosen == d.chosen


@pytest.mark.parametrize("name", ["wave", "numa4", "restricted", "unmatched", "quirk"])
def test_without_devices_it_is_the_reservation_model(name):
    v = V.case(name)
    res, ver, chosen, _, _ = B.dry_run(v.cfg, v.table, v.assigned, v.pdb_allowed, v.pres, None, None, v.base_cfg)
    assert res.tobytes() == v.res.tobytes()
    assert ver.tobytes() == v.verdicts.tobytes()
    assert chosen == v.chosen


# ------------------------------------------------------------- 4. coverage
def test_the_case_set_covers_the_branches():
    cases = {name: B.case(name) for name in B.ALL_CASES}
    total = {}
    for m in cases.values():
        for k, v in m.branches.items():
            total[k] = total.get(k, 0) + v
    for k in B.COVERAGE:
        assert total.get(k, 0) > 0, k
    # ... and the generated cases reach them too, not the hand-worked ones alone
    gen = {k for name in B.CASES for k in cases[name].branches}
    assert set(B.COVERAGE) <= gen
    for slots in B.SLOTS:
        m = cases[f"tiles{slots}"]
        a = m.assigned
        on_resv = np.zeros(m.table.n, bool)
        for q in range(slots):
            on_resv |= (m.table[B.slot_col("resv_flags", q)] & abi.RESV_PRESENT) != 0
        listed = on_resv[a["node"]]
        bound = (a["flags"] & abi.ASG_RESV_SLOT_MASK) != 0
        assert not bound[~listed].any() and 0.35 < bound[listed].mean() < 0.65       # about half are bound
        holds = m.ax["dev_slots"].any(axis=1)
        assert (bound & holds).any() and (~bound & holds).any()
        assert int(np.bincount(a["node"]).max()) == abi.PREEMPT_NODE_PODS            # the node of 128 listed pods
        assert m.table.dev_slots == 8 and m.table.resv_slots == slots
        st = m.verdicts["status"]
        for s in (abi.PREEMPT_CANDIDATE, abi.PREEMPT_UNFIT, abi.PREEMPT_NO_VICTIMS, abi.PREEMPT_UNRESOLVABLE):
            assert (st == s).any(), s
        assert (m.ext["flags"] & abi.PODX_DEVICE).any() and ((m.ext["flags"] & abi.PODX_DEVICE) == 0).sum() >= 2
    nm = cases["numa1"]
    assert nm.numa and (nm.pres["pod"]["flags"] & abi.POD_CPUSET).any()
    assert (nm.verdicts["status"] == abi.PREEMPT_UNRESOLVABLE).any()


# ------------------------------------------------------- 5. the host records
def test_both_tables_stay_parallel():
    """assigned_records with reservation slots skips reserve pods; assigned_ext_records given the same slots does too."""
    prof = with_deviceshare(shipped_profile(reservation=True))
    nodes = {"n0": 0}
    slots = rsv.available_by_node(nodes, [rsv.Reservation(name="a", uid="u-a", node_name="n0")])
    m = D.case("reprieve")

    def pod(name, bound=None, reserve=False, gpu=None):
        ann = {}
        if bound:
            ann[rsv.ANNOTATION_RESERVATION_ALLOCATED] = json.dumps({"uid": bound, "name": "a"})
        if reserve:
            ann[rsv.ANNOTATION_RESERVE_POD] = "true"
        req = {"cpu": k8s.Quantity("1")}
        if gpu is not None:
            ann[deviceshare.ANNOTATION_DEVICE_ALLOCATED] = json.dumps(
                {"gpu": [{"minor": gpu, "resources": {deviceshare.GPU_CORE: "100", deviceshare.GPU_MEMORY_RATIO: "100"}}]})
            req[deviceshare.NVIDIA_GPU] = k8s.Quantity("1")
        return k8s.Pod(name=name, node_name="n0", annotations=ann, containers=[k8s.Container(requests=req)])

    pods = [pod("r", reserve=True), pod("p0", bound="u-a", gpu=1), pod("p1", gpu=0), pod("p2")]
    a, _, keys = pre.assigned_records(pods, prof, nodes, pre.QuotaIds(), reservation_slots=slots)
    ax = pre.assigned_ext_records(pods, m.table, nodes, reservation_slots=slots)
    assert keys == ["default/p0", "default/p1", "default/p2"] and len(ax) == len(a) == 3
    assert (a["flags"] & abi.ASG_RESV_SLOT_MASK).tolist() == [abi.asg_resv_slot(0), 0, 0]
    assert ax["dev_slots"][:, abi.DEV_GPU].tolist() == [1 << 1, 1 << 0, 0]
    k = deviceshare.XRES_INDEX[deviceshare.NVIDIA_GPU]
    assert ax["xreq"][:, k].tolist() == [1, 1, 0]
    assert len(pre.assigned_ext_records(pods, m.table, nodes)) == 4                  # without slots: as before


# --------------------------------------------------------- 6. the constant
PROBE = r"""
#include <stdio.h>
#include "koordhip.h"
int main(void) {
  printf("%u %u %u %u %d\n", KOORDHIP_PREEMPT_NUMA_FROZEN, KOORDHIP_PREEMPT_RESV, KOORDHIP_PREEMPT_DEVICE,
         KOORDHIP_PREEMPT_DEVICE_RESV, KOORDHIP_ABI_VERSION);
  return 0;
}
"""


def test_the_new_constant_matches_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE)
        subprocess.run(["gcc", "-std=c11", "-I", inc, src, "-o", exe], check=True)
        row = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert row == [abi.PREEMPT_NUMA_FROZEN, abi.PREEMPT_RESV, abi.PREEMPT_DEVICE, abi.PREEMPT_DEVICE_RESV, 15]
    assert abi.PREEMPT_DEVICE_RESV == 8 and abi.KOORDHIP_ABI_VERSION == 15
