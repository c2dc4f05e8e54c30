"""The chained decisions of the resolve kernel (k_resolve phase 2c: re-walks,
re-check and closure, and the claim table of the final valid pods, which the
loop builds at its first claimer() probe) on streams that force them: a stream
of c pod classes, so same-class pods collide in every round.  Placements and
the committed node state must equal the CPU oracle's exactly, with every
number of chain passes and with the chain off."""
import functools
import re

import numpy as np
import pytest

import oracle
from koordinator_amd import synth
from koordinator_amd.config import shipped_profile, to_c_config

STATE_KEYS = ("requested", "nz", "npods", "la_used", "la_used_prod")

# chain knobs: the default (one pass), two and three passes, no chain
CHAIN_MODES = [(), (("KOORDHIP_CHAIN_PASSES", "2"),), (("KOORDHIP_CHAIN_PASSES", "3"),), (("KOORDHIP_CHAIN_OFF", "1"),)]
CHAIN_IDS = ["passes-default", "passes-2", "passes-3", "chain-off"]


def class_stream(n_nodes, n_pods, c, numa=False):
    """n_pods records of c classes (record i = class i % c) on n_nodes nodes."""
    prof = shipped_profile(numa=numa)
    table = synth.make_cluster(synth.ClusterSpec(n_nodes), prof)
    if numa:
        synth.add_numa(table, synth.NumaSpec(), prof)
    pods = synth.make_pods(synth.StreamSpec(n_pods, be_frac=0.3, cpuset_frac=0.0), prof)
    pods = pods[np.arange(n_pods) % c].copy()
    return prof, table, pods


@functools.lru_cache(maxsize=None)
def reference(n_nodes, n_pods, c, numa=False):
    """The oracle's placements and final state: computed once per stream, read-only."""
    prof, table, pods = class_stream(n_nodes, n_pods, c, numa)
    o = oracle.Oracle(to_c_config(prof), table)
    ref = o.place_stream(pods)
    ref.setflags(write=False)
    st = {k: np.array(o.state()[k]) for k in STATE_KEYS}
    for v in st.values():
        v.setflags(write=False)
    return ref, st


STREAMS = [(300, 400, 1, False), (300, 400, 2, False), (300, 400, 3, False), (40, 300, 2, False), (10, 300, 2, False),
           (200, 300, 2, True)]


@pytest.mark.parametrize("n_nodes,n_pods,c,numa", STREAMS)
def test_streams_have_c_classes_and_the_oracle_places_them(n_nodes, n_pods, c, numa):
    _, _, pods = class_stream(n_nodes, n_pods, c, numa)
    assert len(np.unique(pods)) == c and len(pods) == n_pods
    ref, _ = reference(n_nodes, n_pods, c, numa)
    assert len(ref) == n_pods and (ref >= 0).sum() > 0
    if n_nodes == 10:  # the pile-up with an unschedulable tail (40 nodes hold all 300 pods of these two classes)
        assert (ref[-40:] < 0).sum() > 10


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def check(Engine, n_nodes, n_pods, c, batch, numa=False):
    prof, table, pods = class_stream(n_nodes, n_pods, c, numa)
    prof.batch_pods = batch
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        got = e.place_stream(pods)
        state = e.read_nodes()
        route = e.kernel_names()["resolve"]
    assert "k_resolve" in route, route
    ref, rs = reference(n_nodes, n_pods, c, numa)
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
    for k in STATE_KEYS:
        assert np.array_equal(state[k], rs[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHAIN_MODES, ids=CHAIN_IDS)
@pytest.mark.parametrize("batch", [8, 24, 64])
@pytest.mark.parametrize("c", [1, 2, 3])
def test_round_sizes_and_pass_counts(Engine, monkeypatch, c, batch, env):
    """400 pods: a short last round at 24 and 64; 64 pods per round reach the
    1 << 64 edges; one class at 24 / 64 gives more than eight conflicting pods."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    check(Engine, 300, 400, c, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHAIN_MODES, ids=CHAIN_IDS)
@pytest.mark.parametrize("n_nodes", [40, 10])
def test_pile_up(Engine, monkeypatch, n_nodes, env):
    """Many pods per node, rounds of 17.  On 10 nodes the stream ends in an
    unschedulable tail: winners with key 0 inside the chain and the re-check
    (40 nodes hold all 300 pods of the two classes)."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    check(Engine, n_nodes, 300, 2, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHAIN_MODES[:3], ids=CHAIN_IDS[:3])
def test_lag_1(Engine, monkeypatch, env):
    """M' is one round: shorter walks over M' entries, other conflicts."""
    monkeypatch.setenv("KOORDHIP_LAG1", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    check(Engine, 300, 400, 2, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHAIN_MODES[:3], ids=CHAIN_IDS[:3])
def test_key_tables_off(Engine, monkeypatch, env):
    """The general path always evaluates: every general-path pod's claimer()
    probes the claim table the loop built."""
    monkeypatch.setenv("KOORDHIP_NO_KEY_TABLES", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    check(Engine, 300, 400, 1, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHAIN_MODES, ids=CHAIN_IDS)
def test_numa_side_rows(Engine, monkeypatch, env):
    """NodeNUMAResource (no cpuset pods: monotone): the chain runs with side rows."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    check(Engine, 200, 300, 2, 16, numa=True)


@pytest.mark.gpu
def test_the_chain_ran(Engine, monkeypatch, capfd):
    """The library's stamps of the one-class stream: pods resolved by the chain,
    and rounds whose claim table the loop built.  (One class at 24 pods per
    round: from the second round on every pod's eight walked entries are M'
    nodes, so all of them take the general path -- the chain resolves pods in
    the first round only, 23 of the 400.)"""
    monkeypatch.setenv("KOORDHIP_STAMPS", "1")
    capfd.readouterr()
    check(Engine, 300, 400, 1, 24)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if "chained decisions:" in ln]
    assert lines, err[-2000:]
    m = re.search(r"(\d+) pods resolved .* rounds with a lazy claim table (\d+)", lines[-1])
    assert m, lines[-1]
    resolved, lazy = (int(x) for x in m.groups())
    assert resolved > 0 and lazy > 0, lines[-1]
