"""The model of the sequential dry run under DeviceShare
(preempt_dev_stream_model.py) on the CPU: the overlay form against the tables
rebuilt from scratch, its two equivalences, the hand-worked cases, the coverage
of the new branches and the stats rule."""
import numpy as np
import pytest

from koordinator_amd import abi

import preempt_dev_model as D
import preempt_dev_stream_model as T
import preempt_stream_model as S


@pytest.mark.parametrize("name", T.ALL_CASES)
def test_overlay_form_is_the_rebuilt_tables(name):
    """case() asserts it for every preemptor: every verdict of every node, the pick, the victims."""
    m = T.case(name)
    assert m.verdicts.shape == (len(m.pres), m.table.n)
    for k in range(len(m.pres)):
        assert (m.res["count"][k] == np.bincount(m.verdicts["status"][k], minlength=abi.PREEMPT_STATUSES)).all()


def test_rebuilt_form_notices_a_wrong_sequence():
    """The second form is no copy of the first's bookkeeping: another victim list for preemptor 0 changes what it
    computes for preemptor 1."""
    m = T.case("share")
    with pytest.raises(AssertionError):
        T.check_rebuilt(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.ext, m.ax, m.numa, m.res,
                        [[], []], m.verdicts)


@pytest.mark.parametrize("name", D.DIRECTED + ("lane",))
def test_one_preemptor_is_the_independent_dry_run(name):
    d = D.case(name)
    res, chosen, stats, ver = T.stream(d.base_cfg, d.table, d.assigned, d.pdb_allowed, d.pres[:1], d.ext[:1], d.ax, d.numa)
    assert res.tobytes() == d.res[:1].tobytes()
    assert ver[0].tobytes() == d.verdicts[0].tobytes()
    assert [int(j) for j in chosen[0]] == [int(j) for j in d.chosen[0]]


@pytest.mark.parametrize("name", ["chain", "prio", "budget", "floor", "word1", "wave"])
def test_empty_records_on_a_device_free_table_are_the_plain_stream(name):
    s = S.case(name)
    res, chosen, stats, _ = T.stream(s.cfg, s.table, s.assigned, s.pdb_allowed, s.pres)
    assert res.tobytes() == s.res.tobytes()
    assert chosen == s.chosen
    assert stats["full_recomputes"] == s.stats["full_recomputes"]


@pytest.mark.parametrize("name", T.HAND)
def test_hand_worked_cases(name):
    m = T.case(name)
    got = [(int(m.res["node"][k]), [int(j) for j in m.chosen[k]]) for k in range(len(m.pres))]
    assert got == T.EXPECTED[name]
    if name in T.EXPECTED_INDEPENDENT:
        res, _, chosen, _, _ = D.dry_run(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.ext, m.ax, m.numa)
        alone = [(int(res["node"][k]), [int(j) for j in chosen[k]]) for k in range(len(m.pres))]
        assert alone == T.EXPECTED_INDEPENDENT[name]
        assert T.claimed_twice(chosen) > 0 and T.claimed_twice(m.chosen) == 0


def test_hand_worked_cases_reach_their_branches():
    want = {
        "reused": ("gone_with_devices", "gone_devices_lowered", "nominated_scalar", "nominated_scalar_blocks"),
        "nodevice_held": ("gone_with_devices", "gone_devices_lowered"),
        "gate": ("nominated_scalar_below_priority", "nominated_scalar", "nominated_scalar_blocks"),
        "share": ("gone_with_devices", "gone_devices_lowered"),
        "twice": ("nominated_scalar",),
        "scalar_gone": ("gone_scalars_only", "nominated_scalar_below_priority"),
        "numa_hand": ("gone_devices_lowered",),
    }
    for name, branches in want.items():
        for b in branches:
            assert T.case(name).branches.get(b, 0) > 0, (name, b)


def test_generated_cases_take_the_new_branches():
    """... all but two: their listed pods hold a scalar only together with a device (`scalar_gone` is that branch),
    and no nominated scalar of theirs turns a fit test (`reused`, `gate` and `twice` are decided by one)."""
    total = {}
    for name in T.GENERATED:
        for b, c in T.case(name).branches.items():
            total[b] = total.get(b, 0) + c
    for b in ("gone_with_devices", "gone_devices_lowered", "gone_without_ext", "nominated_scalar",
              "nominated_scalar_below_priority"):
        assert total.get(b, 0) > 0, (b, total)
    # the sequence does something on them: preemptors share nodes, and no victim is claimed twice
    m = T.case("tiles")
    placed = m.res["node"][m.res["node"] >= 0]
    assert len(placed) > len(set(placed.tolist()))
    assert T.claimed_twice(m.chosen) == 0
    assert T.case("numa").verdicts["status"].max() == abi.PREEMPT_UNRESOLVABLE


def test_stats_rule():
    """The chain's counters from the results: every block, every preemptor; full_recomputes is preempt_stream_model's."""
    m = T.case("tiles")
    assert m.stats == dict(full_recomputes=m.stats["full_recomputes"], block_recomputes=33 * 2, blocks_skipped=0)
    assert T.chain_stats(dict(full_recomputes=3, block_recomputes=9, blocks_skipped=4), 257, 5) == \
        dict(full_recomputes=3, block_recomputes=10, blocks_skipped=0)
    assert T.chain_stats(dict(full_recomputes=0, block_recomputes=0, blocks_skipped=0), 0, 5)["block_recomputes"] == 0
    assert T.case("tiles").stats["full_recomputes"] > 0     # its PDBs and quotas move during the call


def test_the_call_is_exported():
    from koordinator_amd import abi as A
    lib = A.load_library()
    name = "koordhip_preempt_stream_ext"
    assert hasattr(lib, name) and name in A.EXPORTED_SYMBOLS and name in A.ADDITIVE_SYMBOLS
