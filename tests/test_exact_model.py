"""The exact-arithmetic model (exact_model.py) and its edge tables are right:
the model equals the CPU oracle on every generated case and on every case
cluster the GPU tests load (exact_cases.py), and the tables catch the class of
bug they exist for.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle
from koordinator_amd import abi
from koordinator_amd.config import to_c_config

import exact_cases as X
import exact_model as M


def same(got, want, label=lambda i: ""):
    for key in ("status", "scores", "topk"):
        if want.get(key) is None or got.get(key) is None:
            continue
        d = X.first_diff(got[key], want[key])
        assert d is None, (key, d, got[key][d], want[key][d], label(d[-1]))


# ------------------------------------------------------------------ the tables
def test_cap_list_and_table_shape():
    caps = set(M.CAPS)
    assert {1, 3, 7, 100, 1000, 32000, 99, 101, 999, 96001, M.LIMIT - 1, M.LIMIT - 59} <= caps
    for k in (20, 31, 38, 40, 44):
        assert any(0 < c - (1 << k) < 100 for c in caps) and any(0 < (1 << k) - c < 100 for c in caps), k
    assert any(c > 1 << 44 and c % 1000 for c in caps - {M.LIMIT - 1, M.LIMIT - 59})
    for most in (False, True):
        t = M.quotient_edges(most)
        assert len(set(t)) == len(t) and all(abs(r) < M.LIMIT and 0 <= c < M.LIMIT for r, c in t)
        assert any(c == 0 for _, c in t) and any(r < 0 for r, _ in t) and any(r > c > 0 for r, c in t)
        # every cap sees every quotient 0..100, each reached exactly on its boundary
        f = M.most_requested if most else M.least_requested
        for cap in M.CAPS:
            if cap >= 100:
                assert {f(r, c) for r, c in t if c == cap} >= set(range(101)), cap
    assert len(X._qe()[0]) % 64 and len(M.average_grid()) == 10201


def test_scalar_rules_hand_cases():
    assert M.least_requested(0, 0) == 0 and M.least_requested(11, 10) == 0 and M.least_requested(10, 10) == 0
    assert M.least_requested(45600, 96000) == 52 and M.least_requested(0, 10) == 100
    assert M.least_requested(-1, 1) == 200                        # a negative request: no clamp in the reference
    assert M.most_requested(11, 10) == 100 and M.most_requested(0, 0) == 0 and M.most_requested(1, 3) == 33
    assert M.go_div(-7, 2) == -3 and M.go_div(7, -2) == -3 and M.go_div(7, 2) == 3
    assert M.usage_percent(60000, 96000) == 63 and M.usage_percent(1, 200) == 1 and M.usage_percent(29, 200) == 14
    assert M.round_half_away(-2.5) == -3 and M.round_half_away(2.5) == 3 and M.round_half_away(2.4999999) == 2
    assert M.amplify(50, 1.1) == 56 and M.amplify(1000, 1.5) == 1500 and M.amplify(7, 1.0) == 7
    assert M.amplify(3000, 1.1) == 3301 and M.amplify(1000, 1.1) == 1100 and M.amplify(10, 0.5) == 10
    assert M.balanced_score(50, 100, 50, 100) == 100 and M.balanced_score(0, 100, 100, 100) == 50
    assert M.balanced_score(5, 0, 50, 100) == 100
    # a resource with Allocatable 0 leaves both sums; LoadAware keeps its weight
    assert M.weighted_average([(0, 100, 1), (5, 0, 3)]) == 100
    assert M.loadaware_score(0, 5, 100, 0, 0, 0, 1, 3) == 25


def test_model_equals_oracle_scalar_hooks():
    for req, cap in M.quotient_edges(False) + M.quotient_edges(True):
        assert M.least_requested(req, cap) == oracle.least_requested(req, cap), (req, cap)
    for used, total in M.usage_edges():
        assert M.usage_percent(used, total) == oracle.usage_percent(used, total), (used, total)


def test_tables_catch_a_reciprocal_without_fixup():
    """A truncated f * (1/cap rounded to float32) with no fix-up is wrong on
    1441 of the 5483 least-requested cases, and on at least one case of every
    cap >= 2^31; the plain IEEE f64 quotient, truncated, is wrong on none."""
    t = M.quotient_edges()
    wrong = [(r, c) for r, c in t if M.lrs_naive_f32(r, c) != M.least_requested(r, c)]
    print(f"float32 reciprocal, no fix-up: {len(wrong)} of {len(t)} wrong")
    for cap in M.CAPS:
        if cap >= 1 << 31:
            assert any(c == cap for _, c in wrong), cap
    assert len(wrong) >= len(t) // 10
    for r, c in t:
        if c and r <= c:
            assert int(float((c - r) * 100) / float(c)) == M.least_requested(r, c), (r, c)


def test_tables_hold_halves_the_float_rounds_down():
    cases = M.usage_edges()
    down = M.exact_halves_rounded_down(cases)
    print(f"exact halves rounded down by float64: {len(down)}: {down}")
    assert len(down) >= 5
    assert {(29, 200), (57, 200), (113, 200), (145, 1000), (575, 1000)} <= set(down)
    for u, t in down:
        assert M.usage_percent_naive(u, t) == M.usage_percent(u, t) + 1
    # ... and halves it rounds up, and totals whose int64 -> float64 conversion rounds
    assert any(Fraction(u * 100, t).denominator == 2 and M.usage_percent(u, t) == math.ceil(Fraction(u * 100, t))
               for u, t in cases)
    assert any(t > 1 << 53 and int(float(t)) != t for _, t in cases)


def test_wrong_implementations_counted():
    """The device's quotient scheme (reciprocal estimate, truncation, one exact
    fix-up each way) on the tables, with the reciprocal off by up to 2^-26
    either way: right everywhere with both fix-ups; without the upward one
    wrong on hundreds of cases (every exact boundary the estimate falls short
    of); without the downward one wrong wherever the estimate overshoots.
    For the weighted averages (num <= 50000, divisor <= 500, float32) the
    estimate never overshoots a boundary by a whole unit, so only the upward
    fix-up is ever taken: removing the downward one changes no result."""
    t = M.quotient_edges()
    for err in (0.0, 2.0 ** -52, -2.0 ** -52, 2.0 ** -26, -2.0 ** -26):
        for r, c in t:
            assert M.lrs_estimate(r, c, err) == M.least_requested(r, c), (r, c, err)
    no_up = sum(M.lrs_estimate(r, c, -2.0 ** -52, up=False) != M.least_requested(r, c) for r, c in t)
    no_down = sum(M.lrs_estimate(r, c, 2.0 ** -26, down=False) != M.least_requested(r, c) for r, c in t)
    print(f"lrs without the upward fix-up: {no_up} of {len(t)} wrong; without the downward one: {no_down}")
    assert no_up >= 100 and no_down >= 100      # (322 and 1097 of 5483 with this table)
    div_up = div_down = 0
    for ws in (2, 3, 7, 20, 100, 500):
        for num in range(100 * ws + 1):
            for err in (0.0, 2.0 ** -22, -2.0 ** -22):
                assert M.div_weights_estimate(num, ws, err) == num // ws, (num, ws, err)
                div_up += M.div_weights_estimate(num, ws, err, up=False) != num // ws
                div_down += M.div_weights_estimate(num, ws, err, down=False) != num // ws
    print(f"div_weights without the upward fix-up: {div_up} wrong; without the downward one: {div_down}")
    assert div_up > 0 and div_down == 0
    # `> thr` in place of `>= thr`: every node of the usage cluster whose threshold equals its usage
    cases = M.usage_edges()
    assert sum(M.usage_percent(u, tt) > 0 for u, tt in cases) > len(cases) // 2


# ------------------------------------------------------------------ the clusters
@pytest.mark.parametrize("alias", [True, False])
def test_lrs_clusters(alias):
    prof, t, pods = X.lrs_profile(), X.lrs_cluster(alias), X.lrs_pods()
    assert t.n % 64 and t.n % 256
    assert (np.array_equal(t["la_alloc_cpu_m"], t["alloc0"]) and np.array_equal(t["la_alloc_mem"], t["alloc1"])) == alias
    cfg = to_c_config(prof)
    want = X.model_eval(cfg, t, pods, k=16)
    same(oracle.Oracle(cfg, t).eval(pods, k=16), want, X.lrs_label(alias))
    # the loadable cases keep every score inside [0, 100]: what the ranking is sized for
    assert 0 <= want["scores"].min() and 90 < want["scores"].max() <= 100 and (want["topk"]["node"] >= 0).all()
    assert min(int(t[c].min()) for c in t.cols if t[c].dtype == np.int64) == 0


def test_negative_requests_leave_the_score_range():
    """Why the loader refuses a negative quantity: the reference's rule (and
    the oracle) score it above MaxNodeScore, past int32 for a small capacity,
    and below 0 under MostAllocated, where Go truncates toward zero."""
    neg = [(r, c) for r, c in M.quotient_edges() if r < 0 and c]
    assert neg and all(M.least_requested(r, c) > 100 or c > 100 for r, c in neg)
    assert M.least_requested(-1, 1) == 200 == oracle.least_requested(-1, 1)
    assert M.least_requested(-(M.LIMIT - 1), 3) == oracle.least_requested(-(M.LIMIT - 1), 3) > 2**31
    assert M.most_requested(-1, 3) == -33 and M.most_requested(-1, M.LIMIT - 1) == 0
    assert all(r >= 0 and c >= 0 for r, c in M.loadable(M.quotient_edges()))
    assert len(M.quotient_edges()) - len(M.loadable(M.quotient_edges())) == len([1 for r, _ in M.quotient_edges() if r < 0])


def test_mrs_cluster():
    t, pods, label = X.mrs_cluster()
    cfg = to_c_config(X.mrs_profile())
    want = X.model_eval(cfg, t, pods)
    same(oracle.Oracle(cfg, t).eval(pods), want, label)
    mem = {M.most_requested(int(r), int(c)) for r, c in zip(t["requested1"], t["alloc1"])}
    assert set(range(101)) <= mem and int(t["alloc1"].min()) >= 1 << 31
    assert (t["requested1"] >= 0).all() and (want["scores"] >= 0).all()


@pytest.mark.parametrize("fit_w,la_w", X.AVERAGE_ENGINES)
def test_average_clusters(fit_w, la_w):
    t, pods, label = X.average_cluster()
    cfg = to_c_config(X.average_profile(fit_w, la_w))
    want = X.model_eval(cfg, t, pods)
    same(oracle.Oracle(cfg, t).eval(pods), want, label)
    if len(fit_w) == 2:   # every numerator the two-resource average can see
        nums = {fit_w[0] * a + fit_w[1] * b for a, b in M.average_grid()}
        assert len(nums) == 100 * sum(fit_w) + 1 or min(fit_w) > 1


def test_usage_cluster():
    t, cases, where = X.usage_cluster()
    cfg = to_c_config(X.usage_profile())
    pods = X.usage_pods()
    want = X.model_eval(cfg, t, pods)
    label = lambda i: f"(used, total) = {cases[where[i][0]]} on resource {where[i][1]}, prod {cases[where[i][2]]}"
    same(oracle.Oracle(cfg, t).eval(pods, scores=False), {"status": want["status"]}, label)
    la = (want["status"] & abi.ST_LA_FAIL) != 0
    assert not la[2].any()                                  # the DaemonSet pod
    # threshold == usage fails, threshold == usage + 1 passes (a usage of 0 makes threshold 0: skipped)
    for i in range(t.n):
        c, r, pc = where[i]
        u = M.usage_percent(*cases[c])
        assert la[1, i] == (i % 2 == 0 and u != 0), label(i)
        pu = M.usage_percent(cases[pc][0], cases[c][1])
        assert la[0, i] == (i % 2 == 1 and pu != 0), label(i)
    idx, rows, t2 = X.usage_update(t)
    want2 = X.model_eval(cfg, t2, pods)
    same(oracle.Oracle(cfg, t2).eval(pods, scores=False), {"status": want2["status"]}, label)
    flipped = (want2["status"][:, idx] != want["status"][:, idx]).any(axis=0)
    assert flipped.mean() > 0.9


def test_filter_cluster():
    t, rows = X.filter_cluster()
    cfg = to_c_config(X.usage_profile())
    pods = X.filter_pods()
    want = X.model_eval(cfg, t, pods)
    same(oracle.Oracle(cfg, t).eval(pods, scores=False), {"status": want["status"]}, lambda i: rows[i])
    fit = (want["status"] & abi.ST_FIT_FAIL) != 0
    assert fit[0].any() and not fit[0].all() and fit[1].any() and fit[2].sum() == 3


def test_balanced_cluster():
    t, pods, cases = X.balanced_cluster()
    cfg = to_c_config(X.balanced_profile())
    want = X.model_eval(cfg, t, pods)
    same(oracle.Oracle(cfg, t).eval(pods), want, lambda i: cases[i])
    # the table sits on the truncation's edge: exact values that are integers, reached from below by float64
    exact = [100 - Fraction(abs(j - k), 2) for j, _, k, _ in cases[:10201]]
    below = sum(1 for e, s in zip(exact, want["scores"][0, 3, :10201].tolist()) if e.denominator == 1 and s == e - 1)
    assert below >= 5, below


def test_amplify_cluster():
    t, cases = X.amp_cluster()
    cfg = to_c_config(X.mrs_profile())
    pods = X.amp_pods()
    got = oracle.Oracle(cfg, t).eval(pods, scores=False)
    want = status_only(cfg, t, pods)
    d = X.first_diff(got["status"], want)
    assert d is None, (d, cases[d[-1]])
    fail = (want & abi.ST_NUMA_FAIL) != 0
    # slack -1 fails, 0 and +1 pass, for the pod the case is built around
    for i, (ratio, cnt, other, cpu, dd) in enumerate(cases):
        j = X.AMP_POD_CPU.index(cpu)
        assert fail[j, i] == (dd < 0 and ratio > 1), cases[i]
    # a product a hair above an integer is rounded up by a whole unit
    assert M.amplify(50, 1.1) == 56 and float(50) * 1.1 > 55


def status_only(cfg, t, pods):
    """The model's status bits where the Score of a cpuset pod is outside the model."""
    import copy
    c = copy.copy(cfg)
    c.score_plugins = 0
    return X.model_eval(c, t, pods)["status"]


def test_every_device_cluster_is_loadable():
    """Every quantity the GPU tests load lies in [0, 2^45), the loader's range."""
    tables = [X.lrs_cluster(True), X.lrs_cluster(False), X.mrs_cluster()[0], X.average_cluster()[0],
              X.usage_cluster()[0], X.filter_cluster()[0], X.balanced_cluster()[0], X.amp_cluster()[0]]
    tables += [X.stream_cluster(numa, resv) for numa, resv in ((False, False), (True, False), (True, True))]
    cols = ([f"alloc{r}" for r in range(abi.NRES)] + [f"requested{r}" for r in range(abi.NRES)]
            + ["nz_cpu_m", "nz_mem", "la_alloc_cpu_m", "la_alloc_mem", "la_used_cpu_m", "la_used_mem",
               "la_used_prod_cpu_m", "la_used_prod_mem", "resv_alloc0", "resv_alloc1", "resv_nz0", "resv_nz1"])
    for q, t in enumerate(tables):
        for c in cols:
            assert 0 <= int(t[c].min()) and int(t[c].max()) < M.LIMIT, (q, c)
    for p in (X.lrs_pods(), X.usage_pods(), X.filter_pods(), X.amp_pods(), X.stream_pods()):
        for f in ("req", "nz_cpu_m", "nz_mem", "est_cpu", "est_mem"):
            assert 0 <= int(p[f].min()) and int(p[f].max()) < M.LIMIT, f


# ------------------------------------------------------------------ the stream
@pytest.mark.parametrize("numa,resv", [(False, False), (True, False), (True, True)])
def test_stream_cluster_is_not_vacuous(numa, resv):
    prof = X.stream_profile(numa, resv)
    t = X.stream_cluster(numa, resv)
    pods = X.stream_pods(resv=resv)
    placed = oracle.Oracle(to_c_config(prof), t).place_stream(pods)
    print(X.check_stream_not_vacuous(placed))
    assert int(t["alloc1"].max()) == M.LIMIT - 1
