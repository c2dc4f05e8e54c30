"""The NUMA mode's model (preempt_numa_model.py) on the CPU: the generated
cases reach the situations they exist for, the two hand-worked cases give the
verdicts written out beside them, and the premise of the mode holds on every
case: the NodeNUMAResource verdict of a non-amplified node does not depend on
the row.  No GPU."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi
from koordinator_amd.config import shipped_profile, to_c_config, with_upstream

import preempt_model as M
import preempt_numa_model as N

CAND, NOV, UNFIT, ERR, UNRES = range(5)


def cpuset(m):
    return (m.pres["pod"]["flags"] & abi.POD_CPUSET) != 0


def policy_nodes(m):
    return ((m.table["numa_flags"] >> abi.NODE_NUMA_POLICY_SHIFT) & 3) != 0


def fit_only(name):
    """The case's verdicts under the profile without NodeNUMAResource."""
    m = N.case(name)
    prof = with_upstream(shipped_profile()) if name == "static" else shipped_profile()
    return M.dry_run(to_c_config(prof), m.table, m.assigned, m.pdb_allowed, m.pres)


@pytest.mark.parametrize("name", N.ALL_CASES)
def test_every_node_has_one_status(name):
    m = N.case(name)
    assert (m.res["count"].sum(axis=1) == m.table.n).all()
    other = m.verdicts[m.verdicts["status"] != CAND]
    for f in ("n_victims", "n_pdb_violations", "top_priority", "sum_priority", "earliest_start"):
        assert not other[f].any(), f


@pytest.mark.parametrize("name", ["wave", "tiles", "zones8", "static"])
def test_a_unresolvable_by_numa(name):
    """(a) UNRESOLVABLE with the static bit passing."""
    m = N.case(name)
    st = oracle.Oracle(m.cfg, m.table).eval(np.ascontiguousarray(m.pres["pod"]), status=True, scores=False)["status"]
    hit = (m.verdicts["status"] == UNRES) & ((st & abi.ST_STATIC_FAIL) == 0)
    assert hit.any()
    assert not hit[~cpuset(m)].any() or policy_nodes(m).any()   # without policy nodes only a cpuset pod meets the plugin


def test_static_case_has_both_kinds_of_unresolvable():
    m = N.case("static")
    st = oracle.Oracle(m.cfg, m.table).eval(np.ascontiguousarray(m.pres["pod"]), status=True, scores=False)["status"]
    assert ((m.verdicts["status"] == UNRES) & ((st & abi.ST_STATIC_FAIL) != 0)).any()


@pytest.mark.parametrize("name", ["wave", "tiles", "zones8", "static", "frozen"])
def test_b_numa_turns_candidates_away(name):
    """(b) UNFIT or NO_VICTIMS where Fit + LoadAware alone give CANDIDATE."""
    m = N.case(name)
    _, plain, _, _, _ = fit_only(name)
    st = m.verdicts["status"]
    assert (((st == UNFIT) | (st == NOV)) & (plain["status"] == CAND)).any()


@pytest.mark.parametrize("name", ["wave", "tiles", "zones8", "amp"])
def test_c_cpuset_preemptor_with_victims(name):
    """(c) a chosen node with at least one victim for a cpuset preemptor."""
    m = N.case(name)
    assert ((m.res["node"] >= 0) & (m.res["best"]["n_victims"] > 0) & cpuset(m)).any()


@pytest.mark.parametrize("name", ["tiles", "zones8"])
def test_d_policy_nodes_on_both_sides(name):
    """(d) a policy node among the candidates and one among the nodes the frozen verdict fails."""
    m = N.case(name)
    _, plain, _, _, _ = fit_only(name)
    st = m.verdicts["status"]
    pol = policy_nodes(m)[None, :]
    assert ((st == CAND) & pol).any()
    assert (((st == UNFIT) | (st == NOV) | (st == UNRES)) & (plain["status"] == CAND) & pol).any()


def test_e_amp_takes_more_victims():
    """(e) filterAmplifiedCPUs asks for more victims than NodeResourcesFit; the hand-worked lists."""
    m = N.case("amp")
    _, plain, chosen, _, _ = fit_only("amp")
    assert m.chosen == [N.AMP_VICTIMS] and chosen == [N.AMP_FIT_ONLY_VICTIMS]
    assert len(N.AMP_VICTIMS) > len(N.AMP_FIT_ONLY_VICTIMS)
    v = m.verdicts[0, 0]
    # the first victim has priority 7 and start 6; sum over priorities 7 .. 1
    assert tuple(int(v[f]) for f in v.dtype.names) == (CAND, 7, 0, 7, 28 + 7 * (1 << 31), 6)
    assert int(plain[0, 0]["n_victims"]) == 1 and int(plain[0, 0]["top_priority"]) == 1


def test_frozen_cpusets_are_not_freed():
    m = N.case("frozen")
    assert m.verdicts["status"][:, 0].tolist() == [UNFIT, CAND]
    assert m.chosen == [[], N.FROZEN_VICTIMS]
    assert len(m.potential[0][0]) == 4          # all four cpuset pods were removed, and it did not help
    assert m.res["node"].tolist() == [-1, 0]
    s = N.stream_case("frozen")
    assert s.res["node"].tolist() == [-1, 0] and s.chosen == [[], N.FROZEN_VICTIMS]


def test_f_stream_meets_a_nominated_cpuset_preemptor():
    """(f) a later preemptor lands on a node where an earlier cpuset preemptor
    is nominated with a priority that puts it on the row."""
    m, s = N.case("tiles"), N.stream_case("tiles")
    cs, prio, node = cpuset(m), m.pres["priority"], s.res["node"]
    hit = [(j, k) for k in range(len(node)) for j in range(k)
           if node[j] >= 0 and node[j] == node[k] and cs[j] and prio[j] >= prio[k]]
    assert hit


@pytest.mark.parametrize("name", N.ALL_CASES)
def test_stream_of_one_is_the_independent_run(name):
    m = N.case(name)
    res, chosen, _ = N.stream(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres[:1])
    assert res.tobytes() == m.res[:1].tobytes() and chosen == m.chosen[:1]


@pytest.mark.parametrize("name", N.ALL_CASES)
def test_numa_verdict_does_not_move_with_the_row(name):
    """ST_NUMA_FAIL on the loaded rows and on rows stripped of everything, for every non-amplified node."""
    m = N.case(name)
    pods = np.ascontiguousarray(m.pres["pod"])
    loaded = oracle.Oracle(m.cfg, m.table).eval(pods, status=True, scores=False)["status"]
    t = m.table.copy()
    for c in M.ROW_COLS:
        t[c][:] = 0
    stripped = oracle.Oracle(m.cfg, t).eval(pods, status=True, scores=False)["status"]
    plainly = m.table["numa_amp_cpu"] <= 1.0
    assert plainly.any() or name == "amp"       # (its one node is amplified: test_amplified_nodes_do_move)
    assert np.array_equal(loaded[:, plainly] & abi.ST_NUMA_FAIL, stripped[:, plainly] & abi.ST_NUMA_FAIL)


def test_amplified_nodes_do_move():
    """... and on amplified nodes it does: that half of the Filter stays in the walk."""
    m = N.case("amp")
    pods = np.ascontiguousarray(m.pres["pod"])
    t = m.table.copy()
    t["requested0"][:] = 10000
    st = [oracle.Oracle(m.cfg, x).eval(pods, status=True, scores=False)["status"][0, 0] & abi.ST_NUMA_FAIL
          for x in (m.table, t)]
    assert st[0] != 0 and st[1] == 0


def test_the_library_exports_the_call():
    lib = abi.load_library()
    name = "koordhip_preempt_set_mode"
    assert hasattr(lib, name) and name in abi.EXPORTED_SYMBOLS and name in abi.ADDITIVE_SYMBOLS
    assert abi.PREEMPT_NUMA_FROZEN == 1
