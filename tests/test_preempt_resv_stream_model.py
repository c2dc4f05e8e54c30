"""The model of the sequential dry run under Reservation
(preempt_resv_stream_model.py) on the CPU: the overlay form against the tables
rebuilt from scratch, its two equivalences, the hand-worked cases, the coverage
of the named branches and what the sequence is worth on `tiles`."""
import numpy as np
import pytest

from koordinator_amd import abi
from koordinator_amd.snapshot import slot_col

import preempt_model as M
import preempt_resv_model as V
import preempt_resv_stream_model as T
import preempt_stream_model as S


@pytest.mark.parametrize("name", T.ALL_CASES)
def test_overlay_form_is_the_rebuilt_tables(name):
    """case() asserts it for every preemptor: every verdict of every node, the pick, the victims."""
    m = T.case(name)
    assert m.verdicts.shape == (len(m.pres), m.table.n)
    for k in range(len(m.pres)):
        assert (m.res["count"][k] == np.bincount(m.verdicts["status"][k], minlength=abi.PREEMPT_STATUSES)).all()
    nb = (m.table.n + S.BLOCK - 1) // S.BLOCK
    assert m.stats["block_recomputes"] == len(m.pres) * nb and m.stats["blocks_skipped"] == 0


def test_rebuilt_form_notices_a_wrong_sequence():
    """The second form is no copy of the first's bookkeeping: another victim list for preemptor 0 changes what it
    computes for preemptor 1."""
    m = T.case("allocated_freed")
    with pytest.raises(AssertionError):
        T.check_rebuilt(m.cfg, m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.res, [[], []], m.verdicts)


@pytest.mark.parametrize("name", T.DIRECTED)
def test_hand_worked_cases(name):
    m = T.case(name)
    got = [(int(m.res["node"][k]), [int(j) for j in m.chosen[k]]) for k in range(len(m.pres))]
    assert got == T.EXPECTED[name]
    assert m.branches.get(name, 0) > 0, (name, m.branches)        # it reaches the situation it is named for
    if name in T.EXPECTED_INDEPENDENT:
        res, _, chosen, _, _ = V.dry_run(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres, base_cfg=m.base_cfg)
        alone = [(int(res["node"][k]), [int(j) for j in chosen[k]]) for k in range(len(m.pres))]
        assert alone == T.EXPECTED_INDEPENDENT[name]


def test_every_named_branch_is_reached():
    total = {}
    for name in T.ALL_CASES:
        for b, c in T.case(name).branches.items():
            total[b] = total.get(b, 0) + c
    for b in T.NAMED:
        assert total.get(b, 0) > 0, (b, total)
    # the generated cases reach the slots' side on their own
    gen = {b for name in T.GENERATED for b in T.case(name).branches}
    assert {"class_drops", "floor", "nominated_pn", "below_priority"} <= gen, gen


def test_a_cpu_only_slot_keeps_its_memory_allocated():
    """`unmasked`: Mask(requests, ResourceNames) on a slot whose memory Allocated is set to show it."""
    m = T.case("unmasked")
    t = m.table.copy()
    t[slot_col("resv_allocated1", 0)][0] = 5 << 30
    low = T.lowered(t, m.assigned, [0])
    assert int(low[slot_col("resv_allocated1", 0)][0]) == 5 << 30
    assert int(low[slot_col("resv_allocated0", 0)][0]) == 0 and int(low[slot_col("resv_assigned", 0)][0]) == 0


@pytest.mark.parametrize("name", ["wave", "numa", "restricted", "default", "unmatched", "quirk"])
def test_one_preemptor_is_the_independent_dry_run(name):
    d = V.case(name)
    for p in range(min(len(d.pres), 4)):
        res, chosen, stats, ver = T.stream(d.cfg, d.table, d.assigned, d.pdb_allowed, d.pres[p:p + 1], d.base_cfg)
        assert res.tobytes() == d.res[p:p + 1].tobytes()
        assert ver[0].tobytes() == d.verdicts[p].tobytes()
        assert [int(j) for j in chosen[0]] == [int(j) for j in d.chosen[p]]


def test_absent_slots_are_the_plain_stream():
    """No slot present anywhere (and no required affinity, which fails without one): preempt_stream_model.stream
    under the profile without the plugin."""
    d = V.case("wave")
    t = d.table.copy()
    for q in range(max(1, t.resv_slots)):
        t[slot_col("resv_flags", q)][:] = 0
    pres = d.pres.copy()
    pod = pres["pod"]
    pod["flags"] &= ~np.uint32(abi.POD_RESV_AFFINITY)
    pres["pod"] = pod
    res, chosen, stats, _ = T.stream(d.cfg, t, d.assigned, d.pdb_allowed, pres, d.base_cfg)
    want, wchosen, wstats = S.stream(d.base_cfg, t, d.assigned, d.pdb_allowed, pres)
    assert res.tobytes() == want.tobytes()
    assert chosen == wchosen
    assert stats["full_recomputes"] == wstats["full_recomputes"]
    assert (res["node"] >= 0).sum() >= 2


def test_tiles_what_the_sequence_is_worth():
    m, d = T.case("tiles"), V.case("tiles")
    assert T.claimed_twice(m.chosen) == 0
    assert m.res[0].tobytes() == d.res[0].tobytes()
    assert [int(j) for j in m.chosen[0]] == [int(j) for j in d.chosen[0]]
    assert T.claimed_twice(d.chosen) > 0                       # the independent batch does claim pods twice
    assert any(m.gone_bound) and any(m.sees_nominated)


def test_ascending_is_what_the_device_test_needs():
    m = T.case("ascending")
    assert not any(m.sees_nominated)
    assert sum(1 for k in range(1, len(m.pres)) if m.gone_bound[k]) >= 2


def test_the_call_is_exported():
    from koordinator_amd import abi as A
    lib = A.load_library()
    name = "koordhip_preempt_stream_resv"
    assert hasattr(lib, name) and name in A.EXPORTED_SYMBOLS and name in A.ADDITIVE_SYMBOLS
    assert lib.koordhip_abi_version() == 15
