"""The node snapshot's columns through their three paths: load, update rows,
checkpoint / restore.

Every column family the C-ABI loads (LoadAware / Fit, NUMA masks with zone
rows and CPU amplification, static_allow, two reservation slots with reserved
CPUs, DeviceShare rows with device-holding reservations and their scalars,
static Scores, PodTopologySpread and InterPodAffinity counts) is loaded by one
of two profiles: one the pipelined greedy places, one the sequential cycle.
Per profile:

  * update rows equal a fresh load of the updated table (all rows, and a
    shuffled tenth of them);
  * a checkpoint takes every column a Reserve mutates: after a 64-pod stream
    changed each of them, restore brings every read back bit for bit and the
    stream places again as before;
  * a refused update writes nothing.
"""
import functools

import numpy as np
import pytest

from koordinator_amd import abi, synth
from koordinator_amd.config import (shipped_profile, with_deviceshare, with_interpod_affinity, with_normalized_scores,
                                    with_topology_spread, with_upstream)

N, P, SEED = 250, 64, 23
GI = 1 << 30


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


@functools.lru_cache(maxsize=None)
def _workload(kind):
    """(profile, table A, pods, ext or None); treat all of it as read-only."""
    if kind == "greedy":    # the pipelined greedy: no topology-policy node, no ext column
        prof = with_upstream(shipped_profile(numa=True, reservation=True))
        numa = synth.NumaSpec(amp_frac=0.3)
    else:                   # the sequential cycle: every ext family, zone rows on policy nodes
        prof = with_normalized_scores(with_interpod_affinity(with_topology_spread(with_deviceshare(
            with_upstream(shipped_profile(numa=True, reservation=True))))), affinity=1, taint=1)
        numa = synth.NumaSpec(policy_frac=0.4)
    t = synth.make_cluster(synth.ClusterSpec(N, seed=SEED), prof)
    synth.add_numa(t, numa, prof, seed=SEED)
    synth.add_reservations(t, synth.ResvSpec(node_frac=0.8, groups=2, slots=2, multi_frac=0.5,
                                             allocate_once_frac=0.2), seed=SEED)
    synth.add_reserved_cpus(t, frac=0.8, seed=SEED)
    pods = synth.make_pods(synth.StreamSpec(P, be_frac=0.2, seed=SEED, cpuset_frac=0.4, resv_match_frac=0.8,
                                            resv_groups=2), prof)
    ext = None
    if kind == "seq":
        synth.add_devices(t, synth.DevSpec(gpu_frac=0.7), seed=SEED)
        synth.add_device_reservations(t, synth.DevResvSpec(), seed=SEED)
        ext = synth.make_device_ext(P, synth.DevStreamSpec(frac=0.5, seed=SEED))
        synth.add_spread(t, ext, synth.SpreadSpec(seed=SEED))
        synth.add_ipa(t, ext, synth.IpaSpec(seed=SEED))
    synth.add_static(t, pods, synth.StaticSpec(), prof, seed=SEED)
    return prof, t, pods, ext


def _permuted(t):
    """Table B: A's rows in another order, so every family differs on most rows
    while each row stays valid (a hostname domain is the row's own node)."""
    perm = np.random.default_rng(SEED).permutation(t.n)
    b = t.rows(perm)
    b.names = list(t.names)
    if b.has_pts:
        for k in range(b.pts.keys):
            if (b.pts.hostname >> k) & 1:
                d = b["pts_dom"][:, k]
                d[d >= 0] = np.flatnonzero(d >= 0)
    return b


def _reads(e, pods, ext):
    """Every koordhip_read_* the profile allows and the evaluation of a few pods."""
    out = {}
    for name, r in (("nodes", e.read_nodes()), ("numa", e.read_numa()), ("resv", e.read_reservations()),
                    ("dev", e.read_devices())):
        for k, v in r.items():
            out[f"{name}.{k}"] = v
    out["resv_dev"] = e.read_resv_devices()
    out["resv_x"] = e.read_resv_scalars()
    out["pts"] = e.read_pts()
    out["ipa"] = e.read_ipa()
    ev = e.eval(pods[:4], k=4) if ext is None else e.eval_ext(pods[:4], ext[:4], k=4)
    for k in ("status", "scores", "topk"):
        out[f"eval.{k}"] = ev[k]
    return out


def _diff(a, b):
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


def _place(e, pods, ext):
    return e.place_stream(pods) if ext is None else e.place_stream_ext(pods, ext)


# what a 64-pod stream must move, per profile: every read of a column a Reserve mutates
_BASE = ["nodes.requested", "nodes.nz", "nodes.npods", "nodes.la_used", "nodes.la_used_prod", "numa.free",
         "numa.excl_pcpu", "numa.excl_numa", "numa.alloc_cnt", "resv.allocated", "resv.assigned", "resv.cpus"]
MOVED = {
    "greedy": _BASE,
    "seq": _BASE + ["numa.zone_used", "dev.dev_used", "dev.xrequested", "resv_dev", "resv_x", "pts", "ipa"],
}


def test_every_column_family_is_loaded():
    """The two tables together hold a value in every family (a family silently
    absent would let the cases below pass without testing it)."""
    g, s = _workload("greedy")[1], _workload("seq")[1]
    assert g.resv_slots == 2 and s.resv_slots == 2 and s.dev_slots > 0
    for t in (g, s):
        for c in ("alloc0", "requested0", "la_used_cpu_m", "laf_used_m0", "numa_free0", "numa_alloc_cnt",
                  "resv_flags", "resv_flags@1", "resv_alloc0", "resv_allocated0", "resv_assigned", "resv_cpus0"):
            assert t[c].any(), c
        assert (t["numa_class"] >= 0).any() and (t["static_allow"] != 0xFFFFFFFF).any()
        assert t.as_soa().resv_cpus[0]
    assert (g["numa_amp_cpu"] > 1.0).any()
    policy = ((s["numa_flags"] >> abi.NODE_NUMA_POLICY_SHIFT) & 3) != 0
    assert policy.any() and s["numa_zone_alloc"][policy].any() and s["numa_zone_used"][policy].any()
    for c in ("dev_present", "dev_total", "dev_used", "xalloc", "xrequested", "resv_dev", "resv_xalloc",
              "resv_xallocated", "pts_cnt", "pts_elig", "ipa_cnt"):
        assert s[c].any(), c
    assert s["resv_dev"][:, 1].any()
    assert (s["dev_minor"] >= 0).any() and (s["resv_dev_slot"] >= 0).any() and (s["pts_dom"] >= 0).any()
    assert s["static_score"][:, 0].any() and s["static_score"][:, 1].any()
    soa = s.as_soa()
    assert soa.resv_dev_slot and soa.resv_xalloc and soa.static_score[0] and soa.static_score[1] and soa.ipa_cnt


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["greedy", "seq"])
def test_update_rows_equal_a_fresh_load(Engine, kind):
    prof, a, pods, ext = _workload(kind)
    b = _permuted(a)
    rng = np.random.default_rng(SEED + 1)
    some = rng.permutation(a.n)[:a.n // 10]          # shuffled, not sorted
    mixed = a.copy()
    for c in mixed.col_names():
        mixed[c][some] = b[c][some]
    with Engine(prof, device=0) as e:
        e.load_snapshot(b)
        want_all = _reads(e, pods, ext)
        e.load_snapshot(mixed)
        want_some = _reads(e, pods, ext)
        e.load_snapshot(a)
        base = _reads(e, pods, ext)
        assert len(_diff(base, want_all)) > len(base) // 2      # B is another table
        e.update_nodes(some, b.rows(some))
        assert _diff(_reads(e, pods, ext), want_some) == []
        e.load_snapshot(a)
        e.update_nodes(np.arange(a.n), b.rows(np.arange(a.n)))
        assert _diff(_reads(e, pods, ext), want_all) == []


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["greedy", "seq"])
def test_checkpoint_covers_every_mutable_column(Engine, kind):
    prof, a, pods, ext = _workload(kind)
    with Engine(prof, device=0) as e:
        e.load_snapshot(a)
        before = _reads(e, pods, ext)
        e.checkpoint()
        first = _place(e, pods, ext)
        after = _reads(e, pods, ext)
        moved = _diff(before, after)
        print(kind, "placed", int((first >= 0).sum()), "moved", moved)
        assert [k for k in MOVED[kind] if k not in moved] == []
        e.restore()
        assert _diff(_reads(e, pods, ext), before) == []
        again = _place(e, pods, ext)
        assert np.array_equal(first, again)
        assert _diff(_reads(e, pods, ext), after) == []


def _bad_rows(kind, a):
    """(name, indices, rows, message part): one bad value per shared validator."""
    out = []
    r = a.rows([3, 5])
    r["requested0"][1] = 1 << 45
    out.append(("quantity", [3, 5], r, "2^45"))
    if kind != "seq":
        return out
    G = abi.DEV_GPU
    live = (a["dev_minor"][:, G] >= 0) & a["dev_total"][:, G].any(axis=2)
    i = int(np.flatnonzero(live.sum(axis=1) >= 2)[0])
    r = a.rows([i, (i + 1) % a.n])
    r["dev_total"][0, G, int(np.flatnonzero(live[i])[1]), 2] += GI
    out.append(("gpu memory", [i, (i + 1) % a.n], r, "memory sizes"))
    hk = int(a.pts.hostname).bit_length() - 1
    r = a.rows([7, 9])
    r["pts_dom"][0, hk] = 9
    out.append(("hostname", [7, 9], r, "pts_dom out of range"))
    i = int(np.flatnonzero((a["resv_dev_slot"] >= 0) & ((a["resv_flags@1"] & abi.RESV_PRESENT) == 0))[0])
    r = a.rows([i])
    r["resv_dev_slot"][0] = 1
    out.append(("empty slot", [i], r, "names an empty reservation slot"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["greedy", "seq"])
def test_a_refused_update_writes_nothing(Engine, kind):
    prof, a, pods, ext = _workload(kind)
    with Engine(prof, device=0) as e:
        e.load_snapshot(a)
        before = _reads(e, pods, ext)
        for name, idx, rows, part in _bad_rows(kind, a):
            with pytest.raises(abi.KoordhipError) as ei:
                e.update_nodes(idx, rows)
            assert ei.value.code == abi.E_INVAL and part in str(ei.value), (name, str(ei.value))
            assert _diff(_reads(e, pods, ext), before) == [], name
