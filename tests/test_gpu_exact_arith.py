"""The device's exact arithmetic on its edges (eval.hpp's contract): the
quotient fix-ups of lrs / mrs / div_weights, IEEE float64 in the LoadAware
threshold mask, the balanced-allocation score and Amplify, the Filter
comparisons and the host's 2^45 gate.  The edge tables of exact_model.py are
projected one case per node (exact_cases.py); every result must equal both
the Python model and the CPU oracle, bit for bit."""
import numpy as np
import pytest

import oracle
from koordinator_amd import abi
from koordinator_amd.config import to_c_config

import exact_cases as X
import exact_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def agree(got, prof, table, pods, label, k=0, scores=True, model=True):
    """got == the model and got == the oracle; the first differing case is named."""
    cfg = to_c_config(prof)
    refs = [("oracle", oracle.Oracle(cfg, table).eval(pods, scores=scores, k=k))]
    if model:
        mcfg = cfg
        if not scores:
            mcfg = to_c_config(prof)
            mcfg.score_plugins = 0
        refs.append(("model", X.model_eval(mcfg, table, pods, k=k)))
    for name, want in refs:
        for key in ("status", "scores", "topk"):
            if got.get(key) is None:
                continue
            d = X.first_diff(got[key], want[key])
            if d is not None:
                node = int(want[key][d]["node"]) if key == "topk" else d[-1]
                raise AssertionError((name, key, d, f"device {got[key][d]}", f"want {want[key][d]}", label(node)))


# ------------------------------------------------------------------ lrs
def longest_run(v):
    best = run = 1
    for a, b in zip(v[:-1], v[1:]):
        run = run + 1 if a == b else 1
        best = max(best, run)
    return best


def test_lrs_through_fit_and_loadaware_and_ranking(Engine):
    """The quotient-edge table on cpu and memory of Fit and of LoadAware, with
    LoadAware's allocatable aliasing Allocatable and apart from it, non-prod
    and prod usage; and the top 16 over the whole table, whose runs of equal
    totals must come out in ascending node order."""
    prof, pods = X.lrs_profile(), X.lrs_pods()
    with Engine(prof, device=0) as e:
        for alias in (True, False):
            t = X.lrs_cluster(alias)
            e.load_snapshot(t)
            got = e.eval(pods, k=16)
            agree(got, prof, t, pods, X.lrs_label(alias), k=16)
            want = X.model_eval(to_c_config(prof), t, pods, k=16)["topk"]
            tk = got["topk"]
            for j in range(len(pods)):
                # the model's top 16 holds runs of equal totals (5 to 9 long with the aliased columns)
                assert longest_run(want["score"][j].tolist()) >= (5 if alias else 3)
                tie = tk["score"][j][1:] == tk["score"][j][:-1]
                assert (np.diff(tk["node"][j])[tie] > 0).all()


# ------------------------------------------------------------------ mrs
def test_mrs_through_numa_most_allocated(Engine):
    t, pods, label = X.mrs_cluster()
    prof = X.mrs_profile()
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods)
    agree(got, prof, t, pods, label)


def test_negative_quantities_are_refused(Engine):
    """A negative Requested / usage / request scores above MaxNodeScore in the
    reference (200 for (-1, 1); past int32 for -(2^45 - 1) on a small capacity;
    below 0 under MostAllocated): outside the score planes and the totals the
    ranking is sized for, so the host refuses it at every entry point, -1 like
    -2^45, and the context keeps working."""
    prof = X.lrs_profile()
    pods = X.lrs_pods()
    t = X.lrs_cluster(True).rows(np.arange(70))
    assert M.least_requested(-1, 1) == 200 and M.least_requested(-(M.LIMIT - 1), 3) > 2**31
    assert M.most_requested(-1, 3) == -33
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        base = e.eval(pods, k=16)
        for c in QUANTITY_COLS:
            for v in (-1, -(M.LIMIT - 1)):
                bad = t.copy()
                bad[c][69] = v
                refused(lambda: e.update_nodes([69], bad.rows([69])))
        for field, r in POD_QUANTITIES:
            p = pods.copy()
            if r is None:
                p[field][1] = -1
            else:
                p[field][1, r] = -1
            for call in (lambda: e.eval(p), lambda: e.place_stream(p), lambda: e.stage_pods(p),
                         lambda: e.commit(p[1], 0), lambda: e.diagnose(p)):
                refused(call)
        again = e.eval(pods, k=16)
        for key in ("status", "scores", "topk"):
            assert np.array_equal(again[key], base[key]), key
        for c in QUANTITY_COLS:
            bad = t.copy()
            bad[c][0] = -1
            refused(lambda: e.load_snapshot(bad))
        e.load_snapshot(t)
        again = e.eval(pods, k=16)
        for key in ("status", "scores", "topk"):
            assert np.array_equal(again[key], base[key]), key


# ------------------------------------------------------------------ div_weights
@pytest.mark.parametrize("fit_w,la_w", X.AVERAGE_ENGINES)
def test_weighted_averages_over_the_grid(Engine, fit_w, la_w):
    t, pods, label = X.average_cluster()
    prof = X.average_profile(fit_w, la_w)
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods)
    agree(got, prof, t, pods, label)


# ------------------------------------------------------------------ usage_percent
def test_usage_percent_threshold_mask(Engine):
    """Every rounding edge on its threshold (fails) and one under it (passes),
    for a prod, a non-prod and a DaemonSet pod; then a third of the rows
    rewritten with the threshold moved by one (k_prep_flags over a row list)."""
    t, cases, where = X.usage_cluster()
    prof, pods = X.usage_profile(), X.usage_pods()
    label = lambda i: f"(used, total) = {cases[where[i][0]]} on resource {where[i][1]}, prod {cases[where[i][2]]}"
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods, scores=False)
        agree(got, prof, t, pods, label, scores=False)
        idx, rows, t2 = X.usage_update(t)
        e.update_nodes(idx, rows)
        got2 = e.eval(pods, scores=False)
        agree(got2, prof, t2, pods, label, scores=False)
    assert (got2["status"][:, idx] != got["status"][:, idx]).any(axis=0).mean() > 0.9


# ------------------------------------------------------------------ Filter edges
def test_fit_filter_edges(Engine):
    t, rows = X.filter_cluster()
    prof, pods = X.usage_profile(), X.filter_pods()
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods, scores=False)
    agree(got, prof, t, pods, lambda i: rows[i], scores=False)


# ------------------------------------------------------------------ balanced
def test_balanced_allocation_edges(Engine):
    t, pods, cases = X.balanced_cluster()
    prof = X.balanced_profile()
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods)
    agree(got, prof, t, pods, lambda i: cases[i])


# ------------------------------------------------------------------ Amplify
def test_amplified_cpu_filter(Engine):
    t, cases = X.amp_cluster()
    prof, pods = X.mrs_profile(), X.amp_pods()
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.eval(pods, scores=False)
    agree(got, prof, t, pods, lambda i: cases[i], scores=False)


# ------------------------------------------------------------------ the stream
@pytest.mark.parametrize("plugins", ["plain", "fused", "numa", "reservation"])
def test_place_stream_over_the_edges(Engine, monkeypatch, plugins):
    """1500 pods of six awkward sizes on nodes whose cpu / memory columns sit
    on the quotient boundaries (memory caps up to 2^45 - 1): the scan, the
    fused top-k, the class lists and the resolve's re-evaluation of rows it has
    just modified must place like the oracle and leave its node state."""
    if plugins == "fused":
        monkeypatch.setenv("KOORDHIP_EVAL", "fused")
    numa, resv = plugins in ("numa", "reservation"), plugins == "reservation"
    prof, t, pods = X.stream_profile(numa, resv), X.stream_cluster(numa, resv), X.stream_pods(resv=resv)
    o = oracle.Oracle(to_c_config(prof), t)
    ref = o.place_stream(pods)
    X.check_stream_not_vacuous(ref)
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        got = e.place_stream(pods)
        state = e.read_nodes()
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
    rs = o.state()
    for key in ("requested", "nz", "npods", "la_used", "la_used_prod"):
        assert np.array_equal(state[key], rs[key]), key


# ------------------------------------------------------------------ the 2^45 gate
def refused(call):
    with pytest.raises(abi.KoordhipError) as ei:
        call()
    assert ei.value.code == abi.E_INVAL and "2^45" in str(ei.value), str(ei.value)


def gate_table(numa=False, resv=False):
    t = X.stream_cluster(numa, resv).rows(np.arange(9))
    if numa:     # node 4 has a topology policy: its zones are read
        t["numa_flags"][4] = abi.NUMA_TOPO_BEST_EFFORT << abi.NODE_NUMA_POLICY_SHIFT
        t["numa_zone_alloc"][4, 0, :2] = 8000
        t["numa_zone_alloc"][4, 1, :2] = M.LIMIT - 1
    return t


QUANTITY_COLS = ([f"alloc{r}" for r in range(abi.NRES)] + [f"requested{r}" for r in range(abi.NRES)]
                 + ["nz_cpu_m", "nz_mem", "la_alloc_cpu_m", "la_alloc_mem", "la_used_cpu_m", "la_used_mem",
                    "la_used_prod_cpu_m", "la_used_prod_mem"])


def test_exact_range_gate_on_node_columns(Engine):
    """2^45 - 1 is accepted in every quantity column; 2^45 and -2^45 are refused
    at load_snapshot and in an update_nodes row, and the context keeps working."""
    prof = X.stream_profile()
    pods = X.stream_pods(6)
    t = gate_table()
    ok = t.copy()
    for c in QUANTITY_COLS:
        ok[c][7] = M.LIMIT - 1
    with Engine(prof, device=0) as e:
        e.load_snapshot(ok)
        agree(e.eval(pods, k=4), prof, ok, pods, lambda i: i, k=4, model=False)
        e.load_snapshot(t)
        base = e.eval(pods, k=4)
        for c in QUANTITY_COLS:
            for v in (M.LIMIT, -M.LIMIT):
                bad = t.copy()
                bad[c][3] = v
                # a row update: refused before any device write
                refused(lambda: e.update_nodes([3, 5], bad.rows([3, 5])))
                again = e.eval(pods, k=4)
                for key in ("status", "scores", "topk"):
                    assert np.array_equal(again[key], base[key]), (c, v, key)
        for c in QUANTITY_COLS:
            for v in (M.LIMIT, -M.LIMIT):
                bad = t.copy()
                bad[c][3] = v
                refused(lambda: e.load_snapshot(bad))        # (the refused load leaves no snapshot)
                with pytest.raises(abi.KoordhipError) as ei:
                    e.eval(pods)
                assert ei.value.code == abi.E_STATE
                e.load_snapshot(t)
                again = e.eval(pods, k=4)
                for key in ("status", "scores", "topk"):
                    assert np.array_equal(again[key], base[key]), (c, v, key)
        good = t.rows([3, 5])
        good["requested1"][0] = M.LIMIT - 1
        e.update_nodes([3, 5], good)


POD_QUANTITIES = [("req", r) for r in range(abi.NRES)] + [(f, None) for f in ("nz_cpu_m", "nz_mem", "est_cpu", "est_mem")]


def test_exact_range_gate_on_pod_records(Engine):
    """Every quantity of a pod record, through every call that takes one:
    eval, place_stream, stage_pods, commit, uncommit, diagnose, and the pod of
    an assigned-pod record of the preemption dry run."""
    prof = X.stream_profile()
    pods = X.stream_pods(6)
    t = gate_table()

    def with_value(field, r, v):
        p = pods.copy()
        if r is None:
            p[field][2] = v
        else:
            p[field][2, r] = v
        return p

    with Engine(prof, device=0) as e:
        e.load_snapshot(t)
        base = e.eval(pods, k=4)
        big = with_value("req", abi.RES_MEM, M.LIMIT - 1)
        agree(e.eval(big, k=4), prof, t, big, lambda i: i, k=4, model=False)
        asg = np.zeros(3, abi.ASSIGNED_DTYPE)
        asg["pod"] = pods[:3]
        asg["node"] = [0, 1, 2]
        e.preempt_load_pods(asg)
        for field, r in POD_QUANTITIES:
            for v in (M.LIMIT, -M.LIMIT):
                p = with_value(field, r, v)
                refused(lambda: e.eval(p))
                refused(lambda: e.place_stream(p))
                refused(lambda: e.stage_pods(p))
                refused(lambda: e.commit(p[2], 1))
                refused(lambda: e.uncommit(p[2], 1))
                refused(lambda: e.diagnose(p))
                a = asg.copy()
                a["pod"][1] = p[2]
                refused(lambda: e.preempt_load_pods(a))
                again = e.eval(pods, k=4)
                for key in ("status", "scores", "topk"):
                    assert np.array_equal(again[key], base[key]), (field, r, v, key)
        assert np.array_equal(e.read_nodes()["requested"][:, :], np.stack([t[f"requested{r}"] for r in range(abi.NRES)]))


def test_exact_range_gate_on_zones_and_reservations(Engine):
    prof = X.stream_profile(True, True)
    pods = X.stream_pods(6, resv=True)
    t = gate_table(True, True)
    with Engine(prof, device=0) as e:
        e.load_snapshot(t)                       # zone memory of 2^45 - 1 on node 4: accepted
        base = e.eval(pods, k=4)
        ref = oracle.Oracle(to_c_config(prof), t).eval(pods, k=4)
        for key in ("status", "scores", "topk"):
            assert np.array_equal(base[key], ref[key]), key
        bads = []
        for col in ("numa_zone_alloc", "numa_zone_used"):
            for v in (M.LIMIT, -M.LIMIT):
                b = t.copy()
                b[col][4, 1, 1] = v
                bads.append((b, 4))
        for col in ("resv_alloc0", "resv_alloc1", "resv_nz0", "resv_nz1", "resv_allocated0", "resv_allocated1"):
            b = t.copy()
            b[col][5] = M.LIMIT             # node 5 holds a reservation
            bads.append((b, 5))
            b = t.copy()
            b[col][6] = -M.LIMIT            # node 6 holds none: the column is converted all the same
            bads.append((b, 6))
        assert t["resv_flags"][5] and not t["resv_flags"][6]
        for b, node in bads:
            refused(lambda: e.update_nodes([node], b.rows([node])))
            again = e.eval(pods, k=4)
            for key in ("status", "scores", "topk"):
                assert np.array_equal(again[key], base[key]), key
        for b, node in bads:
            refused(lambda: e.load_snapshot(b))
        e.load_snapshot(t)
        again = e.eval(pods, k=4)
        for key in ("status", "scores", "topk"):
            assert np.array_equal(again[key], base[key]), key
