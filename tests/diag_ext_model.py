"""The diagnosis of the sequential-cycle profiles (koordhip_diagnose_ext /
koordhip_node_status_ext), computed with the CPU oracle alone: the cases and,
per pod, the koordhip_diag record of its 16-bit status over the extended Filter
order abi.FILTER_ORDER_EXT.

    Oracle.eval_ext(status)   -> the status bits on the current state
    records()                 -> their histogram, `first` in Filter order
"""
import functools

import numpy as np

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import (shipped_profile, to_c_config, with_deviceshare, with_interpod_affinity,
                                    with_normalized_scores, with_topology_spread, with_upstream)

import diag_model

SEED = synth.SEED

# the (n, n_pods) shapes of full(): one live lane, a partial wave, a ragged
# last node tile with several pod tiles
FULL_SHAPES = [(1, 3), (63, 7), (1003, 70)]


def records(status: np.ndarray) -> np.ndarray:
    """koordhip_diag records of [p][n] 16-bit status words, `first` in the order abi.FILTER_ORDER_EXT."""
    st = np.atleast_2d(status).astype(np.uint32)
    rec = np.zeros(len(st), abi.DIAG_DTYPE)
    rec["feasible"] = (st == 0).sum(axis=1)
    left = np.ones(st.shape, bool)          # nodes no earlier plugin of the Filter order failed
    for bit in abi.FILTER_ORDER_EXT:
        b = bit.bit_length() - 1
        has = (st & bit) != 0
        rec["any"][:, b] = has.sum(axis=1)
        rec["first"][:, b] = (has & left).sum(axis=1)
        left &= ~has
    assert not (st & ~np.uint32(sum(abi.FILTER_ORDER_EXT))).any(), "a status bit outside the Filter order"
    return rec


class Model:
    pass


def _finish(m: Model, stream: bool = False) -> Model:
    """The oracle's status and records on the loaded state and, with `stream`,
    after place_stream_ext of the same pods."""
    m.cfg = to_c_config(m.prof)
    o = oracle.Oracle(m.cfg, m.table)
    m.status = o.eval_ext(m.pods, m.ext, status=True, scores=False)["status"]
    m.rec = records(m.status)
    if stream:
        m.out = o.place_stream_ext(m.pods, m.ext)
        m.status_after = o.eval_ext(m.pods, m.ext, status=True, scores=False)["status"]
        m.rec_after = records(m.status_after)
    return m


@functools.lru_cache(maxsize=None)
def full(n: int, n_pods: int) -> Model:
    """Every sequential-cycle plugin at once: DeviceShare, the extended scalars,
    PodTopologySpread (classes 2 and 4 with a hard hostname constraint),
    InterPodAffinity and the normalized static Scores, with NodeNUMAResource.
    Computed once; callers must not modify it."""
    m = Model()
    m.prof = with_normalized_scores(
        with_interpod_affinity(with_topology_spread(with_deviceshare(shipped_profile(numa=True)))), affinity=1, taint=1)
    m.table = synth.make_cluster(synth.ClusterSpec(n, seed=SEED + 93), m.prof)
    synth.add_numa(m.table, synth.NumaSpec(), m.prof)
    synth.add_devices(m.table, synth.DevSpec())
    m.pods = synth.make_pods(synth.StreamSpec(n_pods, be_frac=0.3, cpuset_frac=0.3), m.prof)
    m.ext = synth.make_device_ext(n_pods, synth.DevStreamSpec(frac=0.4))
    synth.add_spread(m.table, m.ext, synth.SpreadSpec())
    synth.add_ipa(m.table, m.ext, synth.IpaSpec())
    return _finish(m, stream=(n, n_pods) == FULL_SHAPES[-1])


def _resv(spec: synth.ResvSpec, dev_resv: bool) -> Model:
    m = Model()
    m.prof = with_upstream(with_deviceshare(shipped_profile(numa=True, reservation=True)))
    m.table = synth.make_cluster(synth.ClusterSpec(300, seed=SEED + 5), m.prof)
    synth.add_numa(m.table, synth.NumaSpec(), m.prof)
    synth.add_reservations(m.table, spec)
    synth.add_devices(m.table, synth.DevSpec(gpu_frac=0.6))
    if dev_resv:
        synth.add_device_reservations(m.table)
    m.pods = synth.make_pods(synth.StreamSpec(40, be_frac=0.3, cpuset_frac=0.2, resv_match_frac=0.6), m.prof)
    m.ext = synth.make_device_ext(40, synth.DevStreamSpec(frac=0.4))
    synth.add_static(m.table, m.pods, synth.StaticSpec(), m.prof)
    return _finish(m)


@functools.lru_cache(maxsize=None)
def resv() -> Model:
    """Reservations holding devices and extended scalars (the 4-slot rows)."""
    return _resv(synth.ResvSpec(node_frac=0.6), True)


@functools.lru_cache(maxsize=None)
def resv8() -> Model:
    """More than KOORDHIP_RESV_SLOTS reservations on a node (the 8-slot rows)."""
    return _resv(synth.ResvSpec(node_frac=0.6, slots=6, multi_frac=0.6), False)


@functools.lru_cache(maxsize=None)
def plain() -> Model:
    """diag_model's case C inputs, a profile outside the sequential cycle, without ext records."""
    m = Model()
    m.prof, m.table, m.pods = diag_model.inputs(*diag_model.CASES["C"])
    m.ext = None
    return _finish(m)


CASES = {"full-1x3": lambda: full(1, 3), "full-63x7": lambda: full(63, 7), "full-1003x70": lambda: full(1003, 70),
         "resv": resv, "resv8": resv8, "plain": plain}


def first_pods(m: Model, bit: int) -> int:
    """Pods with some node counted first under `bit`."""
    return int((m.rec["first"][:, bit.bit_length() - 1] > 0).sum())


def masked_pods(m: Model, bit: int) -> int:
    """Pods for which `bit` fails on a node an earlier plugin already failed (any != first)."""
    b = bit.bit_length() - 1
    return int((m.rec["any"][:, b] != m.rec["first"][:, b]).sum())
