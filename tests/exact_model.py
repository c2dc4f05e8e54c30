"""A plain high-precision model of the engine's exact arithmetic, and the
deterministic case tables that sit on its edges.

The model is written from the reference's rules (the Go sources the kernels
and the CPU oracle cite), in Python `int` / `fractions.Fraction`; Python
`float` appears only where the reference itself computes in float64
(LoadAware's usage percentage, NodeResourcesBalancedAllocation,
extension.Amplify).  It imports neither the oracle nor the engine: the tests
compare each of them with it.

  leastRequestedScore   loadaware/load_aware.go:388-397,
                        nodenumaresource/least_allocated.go:49-58
  mostRequestedScore    nodenumaresource/most_allocated.go:51-62
  weighted averages     nodenumaresource/scoring.go:191-246 (the koord copy of
                        upstream resource_allocation.go), load_aware.go:378-386
  usage percentage      load_aware.go:214, :248
  Filter                load_aware.go:123-254, reservation/plugin.go:445-494
                        (fitsNode, the mirror of upstream fitsRequest)
  Amplify               apis/extension/node_resource_amplification.go:191-196
  amplified Filter      nodenumaresource/plugin.go:326-363
  balanced allocation   upstream k8s v1.24 balanced_allocation.go
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction

LIMIT = 1 << 45          # the engine's exact range: 0 <= quantity < 2^45
MAX_NODE_SCORE = 100
INT64_MAX = (1 << 63) - 1


# ------------------------------------------------------------------ scalar rules
def go_div(a: int, b: int) -> int:
    """Go's int64 `/`: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def least_requested(req: int, cap: int) -> int:
    if cap == 0:
        return 0
    if req > cap:
        return 0
    return go_div((cap - req) * MAX_NODE_SCORE, cap)


def most_requested(req: int, cap: int) -> int:
    if cap == 0:
        return 0
    if req > cap:
        req = cap
    return go_div(req * MAX_NODE_SCORE, cap)


def weighted_average(terms, scorer=least_requested) -> int:
    """terms: (requested, allocatable, weight) of every resource that counts;
    a resource with Allocatable 0 is left out of both sums."""
    num = ws = 0
    for req, cap, w in terms:
        if cap == 0:
            continue
        num += scorer(req, cap) * w
        ws += w
    return 0 if ws == 0 else go_div(num, ws)


def fit_score(nz_cpu, nz_mem, requested, alloc, pod_nz_cpu, pod_nz_mem, pod_req, weights) -> int:
    """NodeResourcesFit LeastAllocated.  requested / alloc / pod_req / weights:
    five values (cpu, memory, ephemeral-storage, batch-cpu, batch-memory).  cpu
    and memory score NonZeroRequested + the pod's non-zero request; a scalar
    resource (the two batch ones) counts only when the pod requests it."""
    terms = []
    for r, w in enumerate(weights):
        if w == 0:
            continue
        if r == 0:
            terms.append((nz_cpu + pod_nz_cpu, alloc[0], w))
        elif r == 1:
            terms.append((nz_mem + pod_nz_mem, alloc[1], w))
        elif r == 2 or pod_req[r] != 0:
            terms.append((requested[r] + pod_req[r], alloc[r], w))
    return weighted_average(terms)


def loadaware_score(used_cpu, used_mem, alloc_cpu, alloc_mem, est_cpu, est_mem, w_cpu, w_mem, score_zero=False) -> int:
    """loadAwareSchedulingScorer: every configured weight counts in the
    denominator (a resource with Allocatable 0 scores 0 and still weighs)."""
    if score_zero:
        return 0
    num = least_requested(used_cpu + est_cpu, alloc_cpu) * w_cpu + least_requested(used_mem + est_mem, alloc_mem) * w_mem
    return go_div(num, w_cpu + w_mem)


def round_half_away(x: float) -> int:
    """math.Round on a float64, computed on the float itself (x - floor(x) is
    exact for |x| < 2^52)."""
    a = abs(x)
    f = math.floor(a)
    if a - f >= 0.5:
        f += 1
    return -f if x < 0 else f


def usage_percent(used: int, total: int) -> int:
    return round_half_away(float(used) / float(total) * 100.0)


def usage_percent_naive(used: int, total: int) -> int:
    """The exact rational, rounded half up: NOT the reference (it differs on
    the halves the float64 computation rounds down)."""
    return math.floor(Fraction(used * 100, total) + Fraction(1, 2))


def f32(x: float) -> float:
    """x rounded to float32."""
    return struct.unpack("f", struct.pack("f", x))[0]


def lrs_naive_f32(req: int, cap: int) -> int:
    """A WRONG leastRequestedScore: the truncated product with a
    single-precision reciprocal and no remainder fix-up."""
    if cap == 0 or req > cap:
        return 0
    return int(float((cap - req) * 100) * f32(1.0 / cap))


def lrs_estimate(req: int, cap: int, rel_err: float, down: bool = True, up: bool = True) -> int:
    """The device's scheme for leastRequestedScore, with a reciprocal that is
    off by the relative error `rel_err`: the truncated product, then the exact
    remainder fix-up in each direction (`down` / `up` switch one off)."""
    if cap == 0 or req > cap:
        return 0
    f = (cap - req) * 100
    q = int(float(f) * ((1.0 / float(cap)) * (1.0 + rel_err)))
    r = f - q * cap
    if down and r < 0:
        q -= 1
    if up and r >= cap:
        q += 1
    return q


def div_weights_estimate(num: int, ws: int, rel_err: float, down: bool = True, up: bool = True) -> int:
    """The same scheme in float32 for num / ws of the weighted averages."""
    rc = f32(f32(1.0 / ws) * f32(1.0 + rel_err))     # (a product of two float32 is exact in float64)
    q = int(f32(f32(num) * rc))
    r = num - q * ws
    if down and r < 0:
        q -= 1
    if up and r >= ws:
        q += 1
    return q


def usage_ok(used, total, thr) -> bool:
    """One resource of filterNodeUsage / filterProdUsage: True = passes."""
    if thr == 0 or total == 0:
        return True
    return not usage_percent(used, total) >= thr


def balanced_score(req_cpu, alloc_cpu, req_mem, alloc_mem) -> int:
    fr = []
    for req, alloc in ((req_cpu, alloc_cpu), (req_mem, alloc_mem)):
        if alloc == 0:
            continue
        x = float(req) / float(alloc)
        fr.append(1.0 if x > 1 else x)
    std = 0.0
    if len(fr) == 2:
        std = abs((fr[0] - fr[1]) / 2)
    return int((1 - std) * float(MAX_NODE_SCORE))


def amplify(v: int, ratio: float) -> int:
    if ratio <= 1:
        return v
    return int(math.ceil(float(v) * ratio))


def fits_request(npods, alloc_pods, requested, alloc, pod_req, has_req, req_bcpu, req_bmem) -> bool:
    if npods + 1 > alloc_pods:
        return False
    if not has_req:
        return True
    for r in range(3):
        if pod_req[r] > alloc[r] - requested[r]:
            return False
    if req_bcpu and pod_req[3] > alloc[3] - requested[3]:
        return False
    if req_bmem and pod_req[4] > alloc[4] - requested[4]:
        return False
    return True


def amplified_cpu_fits(pod_cpu, cpuset_pod, ratio, allocated_cpus, has_topology, requested_cpu, alloc_cpu) -> bool:
    """filterAmplifiedCPUs: the CPUs held by cpusets count amplified in
    Requested; a cpuset pod's own request is amplified too."""
    if pod_cpu == 0 or ratio <= 1:
        return True
    req = amplify(pod_cpu, ratio) if cpuset_pod else pod_cpu
    allocm = allocated_cpus * 1000 if has_topology else 0
    requested = requested_cpu
    if requested >= allocm and allocm > 0:
        requested = requested - allocm + amplify(allocm, ratio)
    return not req > alloc_cpu - requested


# ------------------------------------------------------------------ case tables
def _pow2_caps():
    out = []
    for k, lo, hi in ((20, 3, 1), (31, 1, 11), (38, 5, 7), (40, 87, 15), (44, 17, 21)):
        out += [(1 << k) - lo, (1 << k) + hi]
    return out


CAPS = ([1, 3, 7, 100, 1000, 32000, 99, 101, 999, 96001] + _pow2_caps()
        + [LIMIT - 1, LIMIT - 59, 31415926535897])
assert all(0 < c < LIMIT for c in CAPS) and len(set(CAPS)) == len(CAPS)


def quotient_edges(most: bool = False, caps=CAPS):
    """(req, cap): for every cap and q in 0..100 the request on, one below and
    one above the boundary where the score steps to q, plus req in {0, cap,
    cap + 1} and cap == 0.  Least-requested boundaries are req = cap -
    ceil(q cap / 100); most-requested ones req = ceil(q cap / 100).  Requests
    of magnitude >= 2^45 are left out.  The table holds negative requests (one
    under the boundary of a full score): the reference's rule and the oracle
    take them, the engine's loader refuses them (`loadable`)."""
    seen, out = set(), []

    def add(req, cap):
        if abs(req) < LIMIT and (req, cap) not in seen:
            seen.add((req, cap))
            out.append((req, cap))

    for cap in caps:
        for q in range(101):
            b = -((-q * cap) // 100)          # ceil(q cap / 100)
            for d in (-1, 0, 1):
                add((b if most else cap - b) + d, cap)
        for req in (0, cap, cap + 1):
            add(req, cap)
    for req in (0, 1, -1, LIMIT - 1):
        add(req, 0)
    return out


def loadable(cases):
    """The (req, cap) cases the engine's loader admits: quantities in [0, 2^45)."""
    return [(r, c) for r, c in cases if 0 <= r < LIMIT and 0 <= c < LIMIT]


def average_grid():
    """(s_cpu, s_mem) over 0..100 x 0..100: with cap = 100 the score of a
    resource is 100 - req, so the grid runs through every numerator the
    two-resource weighted average can see."""
    return [(a, b) for a in range(101) for b in range(101)]


USAGE_TOTALS = [200, 1000, 96000, 64000, 40, 8, 600, 1009, (1 << 40) + 1, (1 << 53) + 1, INT64_MAX]


def usage_edges(totals=USAGE_TOTALS):
    """(used, total): used around every (2k + 1) total / 200, the points where
    the exact percentage is k + 0.5.  The LoadAware filter columns are plain
    int64 on the device with no range limit, so the totals reach past 2^53
    (the int64 -> float64 conversion rounds) up to INT64_MAX."""
    seen, out = set(), []
    for total in totals:
        for k in range(100):
            h = (2 * k + 1) * total // 200
            for d in (-1, 0, 1):
                u = h + d
                if 0 <= u <= INT64_MAX and (u, total) not in seen:
                    seen.add((u, total))
                    out.append((u, total))
    return out


def exact_halves_rounded_down(cases):
    """The cases whose exact percentage is x.5 and whose float64 value rounds down."""
    return [(u, t) for u, t in cases
            if Fraction(u * 100, t).denominator == 2 and usage_percent(u, t) == math.floor(Fraction(u * 100, t))]


def balanced_edges():
    """(req_cpu, alloc_cpu, req_mem, alloc_mem): fractions j / 100 against
    k / 100 make (1 - std) * 100 = 100 - |j - k| / 2, an integer for every even
    difference, which float64 reaches from either side; then other
    denominators, equal fractions, fractions clamped at 1 and an Allocatable
    of 0."""
    out = [(j, 100, k, 100) for j in range(101) for k in range(101)]
    for ac, am in ((50, 200), (3, 7), (1000, 96000), (LIMIT - 1, (1 << 44) + 21), (7, LIMIT - 59)):
        for j in range(0, 51, 5):
            for k in range(0, 51, 7):
                out.append((ac * j // 50, ac, am * k // 50, am))
        over = lambda a: min(a + 1, LIMIT - 1)      # (a request pod pushes a full node over as well)
        out += [(ac, ac, am, am), (over(ac), ac, am // 2, am), (ac // 2, ac, over(am), am), (over(ac), ac, over(am), am)]
    out += [(5, 0, 50, 100), (50, 100, 5, 0), (0, 0, 0, 0), (0, 100, 0, 100)]
    return out


AMP_RATIOS = [1.0, 1.5, 2.0, 1.1, 1.25]


def amplify_edges(pod_cpus=(1000, 50, 3000, 7), cnts=(0, 3, 16)):
    """(ratio, allocated cpus, requested_cpu - held, pod cpu, slack): the
    node's free cpu sits `slack` in {-1, 0, 1} around each pod's amplified
    request.  The requests hold products with the ratio that are integers
    (1000 x 1.5, 1000 x 1.1) and ones a hair above an integer in float64
    (50 x 1.1 = 55.00000000000001 -> 56, 3000 x 1.1 = 3300.0000000000005 ->
    3301, the latter also as 3 CPUs held by cpusets)."""
    out = []
    for ratio in AMP_RATIOS:
        for cnt in cnts:
            for other in (0, 2500):
                for cpu in pod_cpus:
                    for d in (-1, 0, 1):
                        out.append((ratio, cnt, other, cpu, d))
    return out
