"""The resolve kernel's row I/O and round load (kernels.hip: the column-pointer
table in LDS, global_ row loads / write-through stores, load_round's two
trips), at the smallest shapes that reach each of their branches.

Every case runs place_stream on a seeded synth workload and compares the
placements and every read_nodes() column bit for bit with the CPU oracle, and
checks through kernel_stats() / kernel_names() that the intended round shape
and k_resolve build ran.  The oracle's answer is computed once per workload
(shared by the launch-knob cases) and checked not to be vacuous: some pods
placed everywhere, some unschedulable in the pile-up case."""
import functools

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config

pytestmark = pytest.mark.gpu

SEED = 23
COLUMNS = ("requested", "nz", "npods", "la_used", "la_used_prod")


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def build(kind, n_nodes, n_pods):
    """(profile, table, pods) of a workload kind: plain, pileup (plain with
    four pod slots per node, so the stream fills every node), numa or resv."""
    numa = kind in ("numa", "resv")
    prof = shipped_profile(numa=numa, reservation=kind == "resv")
    t = synth.make_cluster(synth.ClusterSpec(n_nodes, seed=SEED), prof)
    if kind == "pileup":
        t["alloc_pods"][:] = t["npods"] + 4
    if numa:
        synth.add_numa(t, synth.NumaSpec(), prof, seed=SEED)
    if kind == "resv":
        synth.add_reservations(t, synth.ResvSpec(node_frac=0.1, groups=4, ordered_frac=0.05), seed=SEED)
        spec = synth.StreamSpec(n_pods, be_frac=0.3, seed=SEED, resv_match_frac=0.2, resv_groups=4)
    else:
        spec = synth.StreamSpec(n_pods, be_frac=0.3, seed=SEED, cpuset_frac=0.4 if numa else 0.0)
    return prof, t, synth.make_pods(spec, prof)


@functools.lru_cache(maxsize=None)
def reference(kind, n_nodes, n_pods):
    """The oracle's placements and final columns (independent of batch_pods
    and of every launch knob: the greedy is sequential)."""
    prof, t, pods = build(kind, n_nodes, n_pods)
    o = oracle.Oracle(to_c_config(prof), t)
    ref = o.place_stream(pods)
    ref.setflags(write=False)
    placed = int((ref != abi.UNSCHEDULABLE).sum())
    assert placed > 0, "vacuous case: the oracle places no pod"
    return ref, o.state(), placed


def run_case(Engine, kind, n_nodes, n_pods, batch, want_lag, want_nm):
    prof, t, pods = build(kind, n_nodes, n_pods)
    prof.batch_pods = batch
    ref, rs, _ = reference(kind, n_nodes, n_pods)
    with Engine(prof, device=0, profile_kernels=True) as e:
        e.load_snapshot(t)
        got = e.place_stream(pods)
        state = e.read_nodes()
        ks = e.kernel_stats()
        name = e.kernel_names()["resolve"]
    assert ks["round_pods"] == batch and ks["lag"] == want_lag, ks
    assert name.startswith("kh::k_resolve<") and name.endswith(", false>"), name
    nm = int(name[len("kh::k_resolve<"):].split(",")[0])
    assert nm in want_nm, name
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
    for c in COLUMNS:
        assert np.array_equal(state[c], rs[c]), c
    return ks


PLAIN = ("plain", 300, 24 * 5 + 7)   # a partial last round at 24 pods per round
NUMA = ("numa", 200, 150)


# 512 threads, three loader waves (192 threads).  Lag 2 lists hold 3P entries:
#   8: 8 x 24 / 2 = 96 list vectors, fewer than loader threads
#   24: the headline's round, 864 vectors
#   32: the largest lag-2 round, 1536 vectors: a second batch in the loop
#   64: the largest round (lag 1, 128 entries): 4096 vectors, 384 pod vectors
@pytest.mark.parametrize("batch,lag", [(8, 2), (24, 2), (32, 2), (64, 1)])
def test_plain_round_sizes(Engine, batch, lag):
    run_case(Engine, *PLAIN, batch, lag, (0,))


def test_fewer_nodes_than_list_entries(Engine):
    """40 nodes under 72-entry lists: short zero-padded lists, pile-ups onto
    the M' nodes, winner rows loaded from HBM, an unschedulable tail."""
    ref, _, placed = reference("pileup", 40, 200)
    assert 0 < placed < len(ref), "the pile-up case needs an unschedulable tail"
    run_case(Engine, "pileup", 40, 200, 24, 2, (0,))


# 256 threads, one loader wave: the side-row pointers and the one-wave list loop
@pytest.mark.parametrize("batch", [16, 5])
def test_numa_one_loader_wave(Engine, batch):
    run_case(Engine, *NUMA, batch, 1, (1,))


def test_reservation_build(Engine):
    """The Reservation side rows (rv columns) of a small snapshot."""
    run_case(Engine, "resv", 200, 120, 8, 2, (3, 4, 5))


# the serial round load, one launch per round (the resumed M' rows go through
# the pointer table at kernel start) and the lag-1 pipeline
@pytest.mark.parametrize("knob,plain_lag", [("KOORDHIP_NO_PRELOAD", 2), ("KOORDHIP_ROUND_LAUNCH", 1), ("KOORDHIP_LAG1", 1)])
@pytest.mark.parametrize("kind", ["plain", "numa"])
def test_launch_knobs(Engine, monkeypatch, knob, plain_lag, kind):
    monkeypatch.setenv(knob, "1")
    if kind == "plain":
        run_case(Engine, *PLAIN, 24, plain_lag, (0,))
    else:
        run_case(Engine, *NUMA, 16, 1, (1,))
