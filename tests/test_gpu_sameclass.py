"""The same-class speculation of the resolve kernel (k_resolve phase 1: a pod
with earlier pods of its class in the round assumes that they take the first
entries outside X of the list they share, and 2b checks that against the
claims) on streams built to reach each of its paths.  Every case compares the
placements and the committed node state with the CPU oracle bit for bit, with
the speculation on and with KOORDHIP_SAMECLS_OFF=1 -- so the two runs agree."""
import functools
import re

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config, with_deviceshare

pytestmark = pytest.mark.gpu

STATE_KEYS = ("requested", "nz", "npods", "la_used", "la_used_prod")
OFF = "KOORDHIP_SAMECLS_OFF"
STAMP = re.compile(r"same-class speculation: made (\d+)  validated (\d+)  invalidated (\d+) \| given up: no head row "
                   r"(\d+)  walk past the entries (\d+)  winner assumed-claimed (\d+)  winner row in HBM (\d+)")
STAMP_KEYS = ("made", "validated", "invalidated", "no_head", "past", "rep", "hbm")


def _classes(prof, n=64):
    """Distinct pod records (classes), in a fixed order."""
    pods = synth.make_pods(synth.StreamSpec(n, be_frac=0.3), prof)
    _, first = np.unique(pods, return_index=True)
    return pods[np.sort(first)]


def stream(n_nodes, n_pods, pattern, tiny=False, rot=0):
    """n_pods records on n_nodes nodes: class pattern[i % len(pattern)] at pod i
    (-1: a class of its own turn, cycling through the classes the letters do
    not use).  tiny: every record requests next to nothing, so a commit does
    not lower a large node's integer score.  rot: pods per round -- the letters
    then stand for other classes in every round (the pool's next ones), so a
    class comes back only after its own commits have left M': the first round
    of a launch never speculates (its ranks are not computed), and a class
    that returned every round would find its list's head covered by M'."""
    prof = shipped_profile()
    table = synth.make_cluster(synth.ClusterSpec(n_nodes), prof)
    if pattern == "mix":  # the generator's own stream: a few dozen classes in random order
        return prof, table, synth.make_pods(synth.StreamSpec(n_pods, be_frac=0.3), prof)
    cls = _classes(prof)
    used = max(pattern) + 1
    assert len(cls) - used >= 24  # (the pods of classes of their own in a round differ)
    idx, spare = [], 0
    for i in range(n_pods):
        p = pattern[i % len(pattern)]
        if rot:  # letters: the round's own classes; -1: the classes after them, one each
            r, j = divmod(i, rot)
            spare = 0 if j == 0 else spare
            if p < 0:
                p = used + spare
                spare += 1
            p = (p + used * r) % len(cls)
        elif p < 0:
            p = used + spare % (len(cls) - used)
            spare += 1
        idx.append(p)
    pods = cls[np.array(idx)].copy()
    if tiny:
        ls = (pods["flags"] & abi.POD_PROD) != 0
        pods["req"][ls, abi.RES_CPU] = 10
        pods["req"][ls, abi.RES_MEM] = 1 << 20
        pods["req"][~ls, abi.RES_BCPU] = 10
        pods["req"][~ls, abi.RES_BMEM] = 1 << 20
        pods["nz_cpu_m"] = 10
        pods["nz_mem"] = 1 << 20
        pods["est_cpu"] = 10
        pods["est_mem"] = 1 << 20
    return prof, table, pods


@functools.lru_cache(maxsize=None)
def reference(n_nodes, n_pods, pattern, tiny=False, rot=0):
    """The oracle's placements and final state: once per stream, read-only."""
    prof, table, pods = stream(n_nodes, n_pods, pattern, tiny, rot)
    o = oracle.Oracle(to_c_config(prof), table)
    ref = o.place_stream(pods)
    ref.setflags(write=False)
    st = {k: np.array(o.state()[k]) for k in STATE_KEYS}
    for v in st.values():
        v.setflags(write=False)
    return ref, st


@pytest.fixture(scope="module")
def Engine():
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    return PlacementEngine


def run(Engine, key, batch):
    prof, table, pods = stream(*key)
    prof.batch_pods = batch
    with Engine(prof, device=0) as e:
        e.load_snapshot(table)
        got = e.place_stream(pods)
        state = e.read_nodes()
        route = e.kernel_names()["resolve"]
    assert "k_resolve" in route, route
    ref, rs = reference(*key)
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
    for k in STATE_KEYS:
        assert np.array_equal(state[k], rs[k]), k
    return got


def check(Engine, monkeypatch, key, batch, env=()):
    """Both runs against the oracle (and so against each other)."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    on = run(Engine, key, batch)
    monkeypatch.setenv(OFF, "1")
    off = run(Engine, key, batch)
    monkeypatch.delenv(OFF)
    assert np.array_equal(on, off)


def stamps(capfd):
    err = capfd.readouterr().err
    found = STAMP.findall(err)
    assert found, err[-2000:]
    return dict(zip(STAMP_KEYS, (int(x) for x in found[-1])))


def check_stamped(Engine, monkeypatch, capfd, key, batch, env=()):
    """check() with the library's stamps: the counters of the run with the
    speculation on; the run with it off makes no speculative decision."""
    monkeypatch.setenv("KOORDHIP_STAMPS", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    on = run(Engine, key, batch)
    s = stamps(capfd)
    monkeypatch.setenv(OFF, "1")
    off = run(Engine, key, batch)
    s_off = stamps(capfd)
    monkeypatch.delenv(OFF)
    assert np.array_equal(on, off)
    assert s_off["made"] == 0 and s_off["validated"] == 0, s_off
    print(s)
    return s


A, B, C, X = 0, 1, 2, -1


@pytest.mark.parametrize("batch", [8, 24, 64])
def test_one_class(Engine, monkeypatch, capfd, batch):
    """One class at 8, 24 and 64 pods per round (another class in every round):
    16, 5 and 2 list-head rows per pod.  At 64 per round a rank of three or
    more has an assumed entry without a head row and gives up."""
    s = check_stamped(Engine, monkeypatch, capfd, (2048, 480, (A,), False, batch), batch)
    assert s["validated"] > 0 and s["made"] == s["validated"] + s["invalidated"], s
    if batch == 64:
        assert s["no_head"] > 0, s


@pytest.mark.parametrize("pattern", [(A, B, A, B), (A, A, B, B), (A, B, B, A), (A, B, C, A, B, C), (A, A, B, B, C, C),
                                     (A, B, C, C, B, A)],
                         ids=["ABAB", "AABB", "ABBA", "ABCABC", "AABBCC", "ABCCBA"])
@pytest.mark.parametrize("n_nodes", [64, 2048])
def test_interleaved_classes(Engine, monkeypatch, capfd, n_nodes, pattern):
    """Two and three classes interleaved: another class's claim falls between
    a pod and its same-class predecessor."""
    s = check_stamped(Engine, monkeypatch, capfd, (n_nodes, 360, pattern, False, 12), 12)
    assert s["made"] == s["validated"] + s["invalidated"], s


@pytest.mark.parametrize("m", [2, 3, 4, 5, 6])
def test_multiplicity(Engine, monkeypatch, capfd, m):
    """m pods of one class in a round of 12, the others of classes of their own."""
    pattern = tuple([A] * (m // 2) + [X] * 3 + [A] * (m - m // 2) + [X] * (9 - m))
    s = check_stamped(Engine, monkeypatch, capfd, (2048, 480, pattern, False, 12), 12)
    assert s["validated"] > 0 and s["made"] == s["validated"] + s["invalidated"], s


def test_tiny_pods_on_large_nodes(Engine, monkeypatch, capfd):
    """A commit that does not lower the node's integer score: the second pod of
    the class wants the same node -- its winner is an assumed-claimed node."""
    s = check_stamped(Engine, monkeypatch, capfd, (256, 240, (A, A, B, A, B, B), True), 12)
    assert s["rep"] > 0, s


@pytest.mark.parametrize("n_nodes,batch", [(20, 8), (40, 12), (70, 24)])
def test_x_covers_the_list(Engine, monkeypatch, n_nodes, batch):
    """Clusters so small that X covers most of a list: M' entries above the
    first free entry, an M' entry winning, walks past the walked entries."""
    check(Engine, monkeypatch, (n_nodes, 300, (A, B, A, A, B, C)), batch)


@pytest.mark.parametrize("pattern", [(A,), (A, B), (A, A, B, A)], ids=["A", "AB", "AABA"])
def test_nearly_full(Engine, monkeypatch, pattern):
    """10 nodes hold a part of the stream: the feasible nodes run out inside a
    round -- one left, the last one taken by a predecessor, rank 1 unschedulable."""
    key = (10, 300, pattern)
    ref, _ = reference(*key)
    assert (ref < 0).sum() > 10 and (ref >= 0).sum() > 10
    check(Engine, monkeypatch, key, 17)


@pytest.mark.parametrize("lag", [1, 2])
def test_lag(Engine, monkeypatch, capfd, lag):
    env = (("KOORDHIP_LAG1", "1"),) if lag == 1 else ()
    s = check_stamped(Engine, monkeypatch, capfd, (2048, 480, (A, B, A, X, X, B, A, X), False, 24), 24, env)
    assert s["validated"] > 0, s


@pytest.mark.parametrize("n_nodes,batch,lag", [(2048, 24, 1), (2048, 24, 2), (2048, 48, 1), (16384, 24, 2)])
def test_mixed_stream(Engine, monkeypatch, capfd, n_nodes, batch, lag):
    """The benchmark stream's shape at test size: some forty classes in random
    order, so most rounds hold a few same-class pairs and triples behind M'
    entries of earlier rounds.  How many of them speculate depends on how far
    the classes' lists share their first nodes (2,048 nodes: 79 made at lag 1,
    21 at lag 2, where M' covers more of the walked entries; 1 at 48 per
    round, 64 given up without a head row), so only the counters' identity is
    asserted; the full-size golden stream speculates in nearly every round."""
    env = (("KOORDHIP_LAG1", "1"),) if lag == 1 else ()
    s = check_stamped(Engine, monkeypatch, capfd, (n_nodes, 960, "mix"), batch, env)
    assert s["made"] == s["validated"] + s["invalidated"], s


def test_the_chain_resolves_what_is_left(Engine, monkeypatch, capfd):
    """Pods of different classes whose lists start with the same nodes still
    conflict: the chained decisions resolve them beside the speculation."""
    monkeypatch.setenv("KOORDHIP_STAMPS", "1")
    capfd.readouterr()
    run(Engine, (2048, 480, (A, B, A, X, X, B, A, X), False, 24), 24)
    err = capfd.readouterr().err
    chain = re.findall(r"chained decisions: \d+ cycles, (\d+) pods resolved", err)
    made = STAMP.findall(err)
    assert chain and made, err[-2000:]
    print("chain resolved", chain[-1], "speculation", made[-1])
    assert int(chain[-1]) > 0 and int(made[-1][1]) > 0


def test_chain_off(Engine, monkeypatch, capfd):
    """No chained decisions, no dependency masks: the speculation is off too."""
    s = check_stamped(Engine, monkeypatch, capfd, (300, 400, (A, B, A)), 24, (("KOORDHIP_CHAIN_OFF", "1"),))
    assert s["made"] == 0 and sum(s.values()) == 0, s


@pytest.mark.parametrize("passes", [1, 2, 3])
def test_chain_passes(Engine, monkeypatch, passes):
    check(Engine, monkeypatch, (2048, 480, (A, B, A, A, C, B), False, 24), 24, (("KOORDHIP_CHAIN_PASSES", str(passes)),))


def test_round_launch(Engine, monkeypatch):
    """One resolve launch per round (no chain bit in its monotone argument):
    the speculation is off on that path."""
    check(Engine, monkeypatch, (300, 240, (A, B, A, A)), 24, (("KOORDHIP_ROUND_LAUNCH", "1"),))


def test_device_pods_between_same_class_pods(Engine, monkeypatch):
    """The mixed DeviceShare stream's shape: device pods (general path, placed
    by the device worker) between the pods of few classes."""
    prof = with_deviceshare(shipped_profile())
    t = synth.make_cluster(synth.ClusterSpec(1500, seed=synth.SEED + 11), prof)
    synth.add_devices(t, synth.DevSpec(), seed=synth.SEED + 11)
    n = 720
    cls = _classes(prof)
    pods = cls[np.array([((A, B, A, A, B, C)[i % 6] + 3 * (i // 24)) % len(cls) for i in range(n)])].copy()
    ext = synth.make_device_ext(n, synth.DevStreamSpec(frac=0.08, seed=synth.SEED + 11))
    dev = (ext["flags"] & abi.PODX_DEVICE) != 0
    assert 20 < dev.sum() < n // 4
    o = oracle.Oracle(to_c_config(prof), t)
    ref = o.place_stream_ext(pods, ext, devices=True)[0]
    ost = o.state()
    got = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(OFF, "1")
        with Engine(prof, device=0) as e:
            e.load_snapshot(t)
            g = e.place_stream_ext(pods, ext)
            route = e.kernel_names()["resolve"]
            st = e.read_nodes()
        assert "k_resolve" in route, route
        assert np.array_equal(g, ref), int(np.flatnonzero(g != ref)[0])
        for k in ("requested", "nz", "npods", "la_used"):
            assert np.array_equal(st[k], ost[k]), k
        got.append(g)
    assert np.array_equal(got[0], got[1]) and (ref[dev] >= 0).sum() > 10
