"""PlacementEngine: the Python face of libkoordhip.so (what the Go shim binds
through cgo).  Thin: every call goes straight to the C-ABI,
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import abi
from .config import Profile, to_c_config
from .snapshot import NodeTable


class PlacementEngine:
    def __init__(self, profile: Profile, device: int = -1, profile_kernels: bool = False):
        self.lib = abi.load_library()
        self.cfg = to_c_config(profile, device)
        self.cfg.profile_kernels = 1 if profile_kernels else 0
        self._ctx = C.c_void_p()
        abi.check(self.lib, self.lib.koordhip_create(C.byref(self.cfg), C.byref(self._ctx)))
        self.n = 0
        self._table: Optional[NodeTable] = None

    def close(self):
        if self._ctx:
            self.lib.koordhip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- snapshot -----------------------------------------------------------
    def load_snapshot(self, table: NodeTable):
        soa = table.as_soa()
        abi.check(self.lib, self.lib.koordhip_load_snapshot(self._ctx, C.byref(soa), table.n))
        self.n = table.n
        self._table = table

    def update_nodes(self, idx, rows: NodeTable):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        soa = rows.as_soa()
        abi.check(self.lib, self.lib.koordhip_update_nodes(self._ctx, abi.ptr(idx, C.c_int32), C.byref(soa), len(idx)))

    def read_nodes(self) -> dict:
        n = self.n
        req = np.zeros((abi.NRES, n), np.int64)
        nz = np.zeros((2, n), np.int64)
        npods = np.zeros(n, np.int32)
        la = np.zeros((2, n), np.int64)
        lap = np.zeros((2, n), np.int64)
        abi.check(self.lib, self.lib.koordhip_read_nodes(self._ctx, abi.ptr(req, C.c_int64), abi.ptr(nz, C.c_int64),
                                                         abi.ptr(npods, C.c_int32), abi.ptr(la, C.c_int64),
                                                         abi.ptr(lap, C.c_int64)))
        return {"requested": req, "nz": nz, "npods": npods, "la_used": la, "la_used_prod": lap}

    # ---- evaluation ---------------------------------------------------------
    def eval(self, pods: np.ndarray, status: bool = True, scores: bool = True, k: int = 0) -> dict:
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        p, n = len(pods), self.n
        st = np.zeros((p, n), np.uint8) if status else None
        sc = np.zeros((p, abi.NPLUGINS, n), np.int32) if scores else None
        tk = np.zeros((p, k), abi.TOPK_DTYPE) if k else None
        abi.check(self.lib, self.lib.koordhip_eval(
            self._ctx, pods.ctypes.data, p, abi.ptr(st, C.c_uint8), abi.ptr(sc, C.c_int32),
            tk.ctypes.data if tk is not None else None, k))
        return {"status": st, "scores": sc, "topk": tk}

    def place_stream(self, pods: np.ndarray) -> np.ndarray:
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        out = np.zeros(len(pods), np.int32)
        abi.check(self.lib, self.lib.koordhip_place_stream(self._ctx, pods.ctypes.data, len(pods),
                                                           abi.ptr(out, C.c_int32)))
        return out

    def place_stream_ext(self, pods: np.ndarray, ext: Optional[np.ndarray] = None) -> np.ndarray:
        """The greedy stream with koordhip_pod_ext records (DeviceShare requests,
        extended scalars); profiles with a normalized Score run the exact
        sequential cycle."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        out = np.zeros(len(pods), np.int32)
        abi.check(self.lib, self.lib.koordhip_place_stream_ext(self._ctx, pods.ctypes.data,
                                                               x.ctypes.data if x is not None else None, len(pods),
                                                               abi.ptr(out, C.c_int32)))
        return out

    def eval_ext(self, pods: np.ndarray, ext: Optional[np.ndarray] = None, status: bool = True, scores: bool = True,
                 k: int = 0) -> dict:
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        p, n = len(pods), self.n
        st = np.zeros((p, n), np.uint16) if status else None
        sc = np.zeros((p, abi.NPLUGINS + abi.NEXT_PLUGINS, n), np.int32) if scores else None
        tk = np.zeros((p, k), abi.TOPK_DTYPE) if k else None
        abi.check(self.lib, self.lib.koordhip_eval_ext(
            self._ctx, pods.ctypes.data, x.ctypes.data if x is not None else None, p, abi.ptr(st, C.c_uint16),
            abi.ptr(sc, C.c_int32), tk.ctypes.data if tk is not None else None, k))
        return {"status": st, "scores": sc, "topk": tk}

    def fetch_devices(self, n: int) -> np.ndarray:
        """[n][DEV_TYPES] device-slot masks the last place call allocated."""
        out = np.zeros((n, abi.DEV_TYPES), np.uint32)
        abi.check(self.lib, self.lib.koordhip_fetch_devices(self._ctx, abi.ptr(out, C.c_uint32), n))
        return out

    def read_devices(self) -> dict:
        S = max(1, self._table.dev_slots if self._table is not None else 0)
        used = np.zeros((self.n, abi.DEV_TYPES, S, abi.DEV_RES), np.int64)
        xr = np.zeros((abi.NXRES, self.n), np.int64)
        abi.check(self.lib, self.lib.koordhip_read_devices(self._ctx, abi.ptr(used, C.c_int64), abi.ptr(xr, C.c_int64)))
        return {"dev_used": used, "xrequested": xr.T.copy()}

    def read_resv_devices(self) -> np.ndarray:
        """The device-holding reservations' column [n][2][TYPES][dev_slots][RES]
        (allocatable, allocated; the allocated half advanced by Reserve)."""
        S = max(1, self._table.dev_slots if self._table is not None else 0)
        out = np.zeros((self.n, 2, abi.DEV_TYPES, S, abi.DEV_RES), np.int64)
        abi.check(self.lib, self.lib.koordhip_read_resv_devices(self._ctx, abi.ptr(out, C.c_int64)))
        return out

    def read_resv_scalars(self) -> np.ndarray:
        """The device-holding reservations' extended-scalar Allocated [n][NXRES]
        (advanced by Reserve; zeros without the resv_xalloc column)."""
        out = np.zeros((abi.NXRES, self.n), np.int64)
        abi.check(self.lib, self.lib.koordhip_read_resv_scalars(self._ctx, abi.ptr(out, C.c_int64)))
        return out.T.copy()

    def read_pts(self) -> np.ndarray:
        """PodTopologySpread matching pods per node and table constraint [n][cons]."""
        m = self._table.pts if self._table is not None else None
        C_ = len(m.cons_key) if m is not None else 0
        out = np.zeros((C_, self.n), np.int32)
        if C_:
            abi.check(self.lib, self.lib.koordhip_read_pts(self._ctx, abi.ptr(out, C.c_int32)))
        return out.T.copy()

    def read_ipa(self) -> np.ndarray:
        """InterPodAffinity count entries' pods per node [n][ents]."""
        m = self._table.ipa if self._table is not None else None
        E = len(m.ent_key) if m is not None else 0
        out = np.zeros((E, self.n), np.int32)
        if E:
            abi.check(self.lib, self.lib.koordhip_read_ipa(self._ctx, abi.ptr(out, C.c_int32)))
        return out.T.copy()

    def stage_pods(self, pods: np.ndarray):
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        self._staged = pods
        abi.check(self.lib, self.lib.koordhip_stage_pods(self._ctx, pods.ctypes.data, len(pods)))

    def stage_pods_ext(self, pods: np.ndarray, ext: Optional[np.ndarray] = None):
        """Stage pods with their koordhip_pod_ext records (the sequential cycle's place_staged)."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        self._staged = pods
        abi.check(self.lib, self.lib.koordhip_stage_pods_ext(self._ctx, pods.ctypes.data,
                                                             x.ctypes.data if x is not None else None, len(pods)))

    def place_staged(self):
        abi.check(self.lib, self.lib.koordhip_place_staged(self._ctx))

    def synchronize(self):
        abi.check(self.lib, self.lib.koordhip_synchronize(self._ctx))

    def fetch_placements(self, n: int) -> np.ndarray:
        out = np.zeros(n, np.int32)
        abi.check(self.lib, self.lib.koordhip_fetch_placements(self._ctx, abi.ptr(out, C.c_int32), n))
        return out

    def checkpoint(self):
        abi.check(self.lib, self.lib.koordhip_checkpoint(self._ctx))

    def restore(self):
        abi.check(self.lib, self.lib.koordhip_restore(self._ctx))

    def commit(self, pod, node: int) -> np.ndarray:
        """Reserve; returns the allocated cpuset mask (zeros for a non-cpuset pod).
        Raises KoordhipError(code=abi.E_RESERVE) when the NUMA Allocate fails."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        cpus = np.zeros(abi.NUMA_WORDS, np.uint64)
        abi.check(self.lib, self.lib.koordhip_commit(self._ctx, pod.ctypes.data, int(node),
                                                     abi.ptr(cpus, C.c_uint64)))
        return cpus

    def uncommit(self, pod, node: int, cpus=None):
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        c = None if cpus is None else np.ascontiguousarray(cpus, dtype=np.uint64)
        abi.check(self.lib, self.lib.koordhip_uncommit(self._ctx, pod.ctypes.data, int(node),
                                                       abi.ptr(c, C.c_uint64)))

    def commit_ext(self, pod, ext, node: int):
        """Reserve of one pod with its koordhip_pod_ext record (DeviceShare, the
        extended scalars, PodTopologySpread / InterPodAffinity counts besides
        koordhip_commit's plugins): returns (cpus [NUMA_WORDS], device slots [DEV_TYPES])."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        x = np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        cpus = np.zeros(abi.NUMA_WORDS, np.uint64)
        dev = np.zeros(abi.DEV_TYPES, np.uint32)
        abi.check(self.lib, self.lib.koordhip_commit_ext(self._ctx, pod.ctypes.data, x.ctypes.data, int(node),
                                                         abi.ptr(cpus, C.c_uint64), abi.ptr(dev, C.c_uint32)))
        return cpus, dev

    def uncommit_ext(self, pod, ext, node: int, cpus=None, dev=None):
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        x = np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        c = None if cpus is None else np.ascontiguousarray(cpus, dtype=np.uint64)
        d = None if dev is None else np.ascontiguousarray(dev, dtype=np.uint32)
        abi.check(self.lib, self.lib.koordhip_uncommit_ext(self._ctx, pod.ctypes.data, x.ctypes.data, int(node),
                                                           abi.ptr(c, C.c_uint64), abi.ptr(d, C.c_uint32)))

    def read_numa(self) -> dict:
        n = self.n
        fr = np.zeros((abi.NUMA_WORDS, n), np.uint64)
        ep = np.zeros((abi.NUMA_WORDS, n), np.uint64)
        en = np.zeros((abi.NUMA_WORDS, n), np.uint64)
        cnt = np.zeros(n, np.int32)
        abi.check(self.lib, self.lib.koordhip_read_numa(self._ctx, abi.ptr(fr, C.c_uint64), abi.ptr(ep, C.c_uint64),
                                                        abi.ptr(en, C.c_uint64), abi.ptr(cnt, C.c_int32)))
        zu = np.zeros((n, 2, abi.NUMA_MAX_NODES), np.int64)
        abi.check(self.lib, self.lib.koordhip_read_numa_zones(self._ctx, abi.ptr(zu, C.c_int64)))
        return {"free": fr, "excl_pcpu": ep, "excl_numa": en, "alloc_cnt": cnt, "zone_used": zu}

    def read_reservations(self) -> dict:
        """Reservation mutable state: Allocated [2][S n] (cpu milli, memory), len(AssignedPods) [S n],
        S = the loaded table's reservation slots, slot-major."""
        n = self.n * max(1, self._table.resv_slots)
        al = np.zeros((2, n), np.int64)
        asg = np.zeros(n, np.int32)
        abi.check(self.lib, self.lib.koordhip_read_reservations(self._ctx, abi.ptr(al, C.c_int64), abi.ptr(asg, C.c_int32)))
        rc = np.zeros((abi.NUMA_WORDS, n), np.uint64)
        abi.check(self.lib, self.lib.koordhip_read_resv_cpus(self._ctx, abi.ptr(rc, C.c_uint64)))
        return {"allocated": al, "assigned": asg, "cpus": rc}

    def fetch_cpusets(self, n: int) -> np.ndarray:
        out = np.zeros((n, abi.NUMA_WORDS), np.uint64)
        abi.check(self.lib, self.lib.koordhip_fetch_cpusets(self._ctx, abi.ptr(out, C.c_uint64), n))
        return out

    # ---- why a pod is unschedulable (koordinator_amd.diagnosis reads the records)
    def diagnose(self, pods: np.ndarray) -> np.ndarray:
        """Per-plugin node counts (abi.DIAG_DTYPE records) of `pods` against the
        current state; stateless, no commit."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        out = np.zeros(len(pods), abi.DIAG_DTYPE)
        abi.check(self.lib, self.lib.koordhip_diagnose(self._ctx, pods.ctypes.data, len(pods), out.ctypes.data))
        return out

    def diagnose_ext(self, pods: np.ndarray, ext: Optional[np.ndarray] = None) -> np.ndarray:
        """diagnose() for every profile and snapshot, the sequential cycle's
        included (DeviceShare, the extended scalars, PodTopologySpread,
        InterPodAffinity): records whose `first` follows abi.FILTER_ORDER_EXT."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        out = np.zeros(len(pods), abi.DIAG_DTYPE)
        abi.check(self.lib, self.lib.koordhip_diagnose_ext(self._ctx, pods.ctypes.data,
                                                           x.ctypes.data if x is not None else None, len(pods),
                                                           out.ctypes.data))
        return out

    def node_status_ext(self, pod, ext=None) -> np.ndarray:
        """[n] 16-bit abi.ST_* status words of one pod against the current
        state: eval_ext's status row without its planes."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        if len(pod) != 1 or (x is not None and len(x) != 1):
            raise ValueError("node_status_ext takes one pod")
        out = np.zeros(self.n, np.uint16)
        abi.check(self.lib, self.lib.koordhip_node_status_ext(self._ctx, pod.ctypes.data,
                                                              x.ctypes.data if x is not None else None,
                                                              abi.ptr(out, C.c_uint16)))
        return out

    def fetch_diagnosis(self, n: int) -> np.ndarray:
        """The records of the last place call's unplaced pods (out_node < 0) at
        the state each was decided on; all-zero records for placed pods."""
        out = np.zeros(n, abi.DIAG_DTYPE)
        abi.check(self.lib, self.lib.koordhip_fetch_diagnosis(self._ctx, out.ctypes.data, n))
        return out

    def fetch_node_status(self, pod_index: int) -> np.ndarray:
        """[n] abi.ST_* status bytes of one unplaced pod of the last place call
        at its decision state (the PostFilter NodeToStatusMap)."""
        out = np.zeros(self.n, np.uint8)
        abi.check(self.lib, self.lib.koordhip_fetch_node_status(self._ctx, int(pod_index), abi.ptr(out, C.c_uint8)))
        return out

    # ---- ... and the FitError reasons per node (abi.REASON_*; diagnosis.fit_error_message reads the records)
    def diagnose_reasons(self, pods: np.ndarray) -> np.ndarray:
        """Per-reason node counts (abi.REASONS_DTYPE records) of `pods` against
        the current state; diagnose()'s envelope, stateless, no commit."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        out = np.zeros(len(pods), abi.REASONS_DTYPE)
        abi.check(self.lib, self.lib.koordhip_diagnose_reasons(self._ctx, pods.ctypes.data, len(pods), out.ctypes.data))
        return out

    def node_reasons(self, pod) -> np.ndarray:
        """[n] 32-bit abi.REASON_* masks of one pod against the current state:
        the reasons of every failing plugin on each node."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        if len(pod) != 1:
            raise ValueError("node_reasons takes one pod")
        out = np.zeros(self.n, np.uint32)
        abi.check(self.lib, self.lib.koordhip_node_reasons(self._ctx, pod.ctypes.data, abi.ptr(out, C.c_uint32)))
        return out

    def fetch_reasons(self, n: int) -> np.ndarray:
        """fetch_diagnosis() with reason records: the last place call's unplaced
        pods at their decision states; all-zero records for placed pods."""
        out = np.zeros(n, abi.REASONS_DTYPE)
        abi.check(self.lib, self.lib.koordhip_fetch_reasons(self._ctx, out.ctypes.data, n))
        return out

    def fetch_node_reasons(self, pod_index: int) -> np.ndarray:
        """fetch_node_status() with reason masks: [n] abi.REASON_* masks of one
        unplaced pod of the last place call at its decision state."""
        out = np.zeros(self.n, np.uint32)
        abi.check(self.lib, self.lib.koordhip_fetch_node_reasons(self._ctx, int(pod_index), abi.ptr(out, C.c_uint32)))
        return out

    def diagnose_reasons_ext(self, pods: np.ndarray, ext: Optional[np.ndarray] = None) -> np.ndarray:
        """diagnose_reasons() for every profile and snapshot diagnose_ext()
        answers for: abi.REASONS_DTYPE records with slots 19-31 filled
        (DeviceShare, the extended scalars, PodTopologySpread,
        InterPodAffinity), `first` and `unresolvable` as abi.first_reasons_ext
        and abi.REASON_EXT_UNRESOLVABLE_MASK give them."""
        pods = np.ascontiguousarray(pods, dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(ext, dtype=abi.POD_EXT_DTYPE)
        out = np.zeros(len(pods), abi.REASONS_DTYPE)
        abi.check(self.lib, self.lib.koordhip_diagnose_reasons_ext(self._ctx, pods.ctypes.data,
                                                                   x.ctypes.data if x is not None else None, len(pods),
                                                                   out.ctypes.data))
        return out

    def node_reasons_ext(self, pod, ext=None) -> np.ndarray:
        """[n] 32-bit abi.REASON_* masks of one pod against the current state,
        the sequential cycle's plugins included; abi.reasons_status_ext of it
        is node_status_ext's row."""
        pod = np.ascontiguousarray(np.atleast_1d(pod), dtype=abi.POD_DTYPE)
        x = None if ext is None else np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        if len(pod) != 1 or (x is not None and len(x) != 1):
            raise ValueError("node_reasons_ext takes one pod")
        out = np.zeros(self.n, np.uint32)
        abi.check(self.lib, self.lib.koordhip_node_reasons_ext(self._ctx, pod.ctypes.data,
                                                               x.ctypes.data if x is not None else None,
                                                               abi.ptr(out, C.c_uint32)))
        return out

    # ---- preemption dry run (koordinator_amd.preemption builds the records)
    def preempt_load_pods(self, assigned: np.ndarray, pdb_allowed=(), ext=None):
        """Upload the table of the pods that sit on the nodes (abi.ASSIGNED_DTYPE)
        and the PDBs' DisruptionsAllowed; valid until the next call or load_snapshot.
        ext: abi.ASSIGNED_EXT_DTYPE records beside them (the extended scalars and
        devices the pods hold, preemption.assigned_ext_records), read by the dry
        run under DeviceShare (preempt_set_mode(device=True))."""
        a = np.ascontiguousarray(assigned, dtype=abi.ASSIGNED_DTYPE)
        pdb = np.ascontiguousarray(pdb_allowed, dtype=np.int32)
        if ext is None:
            abi.check(self.lib, self.lib.koordhip_preempt_load_pods(self._ctx, a.ctypes.data, len(a),
                                                                    abi.ptr(pdb, C.c_int32), len(pdb)))
            return
        x = np.ascontiguousarray(ext, dtype=abi.ASSIGNED_EXT_DTYPE)
        if len(x) != len(a):
            raise ValueError("preempt_load_pods: one ext record per assigned pod")
        self._need("koordhip_preempt_load_pods_ext")
        abi.check(self.lib, self.lib.koordhip_preempt_load_pods_ext(self._ctx, a.ctypes.data, x.ctypes.data, len(a),
                                                                    abi.ptr(pdb, C.c_int32), len(pdb)))

    def _need(self, symbol: str):
        if not hasattr(self.lib, symbol):
            raise RuntimeError(f"this libkoordhip build has no {symbol}")

    EXT_NULL = object()   # preempt_stream(ext=EXT_NULL): koordhip_preempt_stream_ext with ext == NULL

    def _pre_ext(self, ext, n: int):
        if ext is None:
            return None
        x = np.ascontiguousarray(np.atleast_1d(ext), dtype=abi.POD_EXT_DTYPE)
        if len(x) != n:
            raise ValueError("one koordhip_pod_ext record per preemptor")
        return x

    def preempt_set_mode(self, numa_frozen: bool = False, resv: bool = False, flags: int = None, device: bool = False,
                         device_resv: bool = False):
        """numa_frozen: the dry-run calls accept NodeNUMAResource in the Filter,
        with the plugin's verdict frozen for the call: victims' cpusets and
        zone amounts are not freed and a nominated cpuset preemptor holds no
        CPUs, as in the reference (include/koordhip.h).  resv: preempt() and
        preempt_node_verdicts() accept Reservation state: the walk starts from
        the restored row and keeps the plugin's AddPod / RemovePod state
        (listed pods name their reservation slot, preemption.assigned_records);
        preempt_stream() still refuses it (preempt_stream(resv=True) is the
        mode's sequential dry run).  The shipped profile needs both;
        on a profile with NodeNUMAResource in the Filter and without the
        Reservation plugin resv=True is refused (KOORDHIP_EINVAL).
        device: preempt() and preempt_node_verdicts() accept a profile whose
        sequential-cycle plugins are DeviceShare only: victims' extended scalars
        and devices are freed in the walk (preempt_load_pods(ext=...), the
        preemptors' records as preempt(ext=...)); refused on a profile without
        DeviceShare, with PodTopologySpread / InterPodAffinity or Reservation
        state, and by preempt_stream() without ext (preempt_stream(ext=...) is
        the mode's sequential dry run).
        device_resv: the opt-in for DeviceShare beside Reservation state, only
        together with resv=True and device=True (and numa_frozen=True where
        NodeNUMAResource filters: the shipped profile with DeviceShare needs
        all four) and on a profile that has both plugins, KOORDHIP_EINVAL
        elsewhere: preempt() and preempt_node_verdicts() then accept cpu /
        memory reservations beside device columns, listed pods that name a slot
        and have an ext record; a bound victim's devices are not freed, the
        plugin's maps carry the extended scalars (include/koordhip.h).
        Device-holding reservations and preempt_stream() stay refused.
        The mode is the context's; False restores the refusal.  flags: the raw
        abi.PREEMPT_* word instead."""
        if not hasattr(self.lib, "koordhip_preempt_set_mode"):
            raise RuntimeError("this libkoordhip build has no koordhip_preempt_set_mode")
        word = ((abi.PREEMPT_NUMA_FROZEN if numa_frozen else 0) | (abi.PREEMPT_RESV if resv else 0) |
                (abi.PREEMPT_DEVICE if device else 0) |
                (abi.PREEMPT_DEVICE_RESV if device_resv else 0)) if flags is None else int(flags)
        abi.check(self.lib, self.lib.koordhip_preempt_set_mode(self._ctx, word))

    def preempt(self, preemptors: np.ndarray, max_victims: int = 0, ext=None):
        """SelectVictimsOnNode on every node and the candidate pick, per
        preemptor (abi.PREEMPTOR_DTYPE) against the current state: returns
        (abi.PREEMPT_RESULT_DTYPE [p], victims [p][max_victims] as indices into
        the loaded table, -1 padded).  Writes no engine state.  ext: the
        preemptors' abi.POD_EXT_DTYPE records (the DeviceShare mode; None: no
        device or extended-scalar request)."""
        pre = np.ascontiguousarray(np.atleast_1d(preemptors), dtype=abi.PREEMPTOR_DTYPE)
        out = np.zeros(len(pre), abi.PREEMPT_RESULT_DTYPE)
        vic = np.full((len(pre), max_victims), -1, np.int32)
        x = self._pre_ext(ext, len(pre))
        if x is None:
            abi.check(self.lib, self.lib.koordhip_preempt(self._ctx, pre.ctypes.data, len(pre), out.ctypes.data,
                                                          abi.ptr(vic, C.c_int32) if max_victims else None, max_victims))
        else:
            self._need("koordhip_preempt_ext")
            abi.check(self.lib, self.lib.koordhip_preempt_ext(self._ctx, pre.ctypes.data, x.ctypes.data, len(pre),
                                                              out.ctypes.data,
                                                              abi.ptr(vic, C.c_int32) if max_victims else None,
                                                              max_victims))
        return out, vic

    def preempt_stream(self, preemptors: np.ndarray, max_victims: int = 0, ext=None, resv: bool = False):
        """The dry run of a batch whose answers hold together: the preemptors
        are processed in input order, each on the state the earlier ones left
        (their victims gone, they themselves nominated on their nodes, PDB
        budgets and their quotas' used lowered; include/koordhip.h).  Every
        q_used is as of the start of the call.  Returns (results, victims,
        stats) with stats a dict of koordhip_preempt_stream_stats.  Writes no
        engine state and leaves the loaded table as it was.  ext: the
        preemptors' abi.POD_EXT_DTYPE records: koordhip_preempt_stream_ext, the
        sequential dry run of the DeviceShare mode (gone victims' scalars and
        devices are off their nodes, nominated preemptors' scalars on them and
        a nominated pod holds no device); EXT_NULL: that call with all-empty
        records; None: the plain call, which a DeviceShare profile refuses.
        resv=True: koordhip_preempt_stream_resv, the sequential dry run of the
        Reservation mode (preempt_set_mode(resv=True)): gone victims also leave
        their reservations' Allocated and assigned counts, and a nominated
        preemptor moves the plugin's state as in the reference's two Filter
        passes; the plain call keeps refusing Reservation
        state.  Not together with ext (ValueError)."""
        if resv and ext is not None:
            raise ValueError("preempt_stream: resv=True takes no ext records (the DEVICE mode beside Reservation "
                             "state is not built)")
        pre = np.ascontiguousarray(np.atleast_1d(preemptors), dtype=abi.PREEMPTOR_DTYPE)
        out = np.zeros(len(pre), abi.PREEMPT_RESULT_DTYPE)
        vic = np.full((len(pre), max_victims), -1, np.int32)
        st = np.zeros(1, abi.PREEMPT_STREAM_STATS_DTYPE)
        pv = abi.ptr(vic, C.c_int32) if max_victims else None
        if resv:
            self._need("koordhip_preempt_stream_resv")
            abi.check(self.lib, self.lib.koordhip_preempt_stream_resv(self._ctx, pre.ctypes.data, len(pre),
                                                                      out.ctypes.data, pv, max_victims, st.ctypes.data))
        elif ext is None:
            abi.check(self.lib, self.lib.koordhip_preempt_stream(self._ctx, pre.ctypes.data, len(pre), out.ctypes.data,
                                                                 pv, max_victims, st.ctypes.data))
        else:
            self._need("koordhip_preempt_stream_ext")
            x = None if ext is self.EXT_NULL else self._pre_ext(ext, len(pre))
            abi.check(self.lib, self.lib.koordhip_preempt_stream_ext(self._ctx, pre.ctypes.data,
                                                                     None if x is None else x.ctypes.data, len(pre),
                                                                     out.ctypes.data, pv, max_victims, st.ctypes.data))
        return out, vic, {f: int(st[f][0]) for f in st.dtype.names}

    def preempt_node_verdicts(self, preemptor, ext=None) -> np.ndarray:
        """One preemptor's verdict on every node (abi.PREEMPT_NODE_DTYPE [n]).
        ext: its abi.POD_EXT_DTYPE record (the DeviceShare mode)."""
        pre = np.ascontiguousarray(np.atleast_1d(preemptor), dtype=abi.PREEMPTOR_DTYPE)
        if len(pre) != 1:
            raise ValueError("preempt_node_verdicts takes one preemptor")
        out = np.zeros(self.n, abi.PREEMPT_NODE_DTYPE)
        x = self._pre_ext(ext, 1)
        if x is None:
            abi.check(self.lib, self.lib.koordhip_preempt_node_verdicts(self._ctx, pre.ctypes.data, out.ctypes.data))
        else:
            self._need("koordhip_preempt_node_verdicts_ext")
            abi.check(self.lib, self.lib.koordhip_preempt_node_verdicts_ext(self._ctx, pre.ctypes.data, x.ctypes.data,
                                                                            out.ctypes.data))
        return out

    def last_stats(self) -> dict:
        em, tm = C.c_double(), C.c_double()
        nl, ne = C.c_int64(), C.c_int64()
        abi.check(self.lib, self.lib.koordhip_last_stats(self._ctx, C.byref(em), C.byref(nl), C.byref(ne), C.byref(tm)))
        return {"eval_ms": em.value, "eval_launches": nl.value, "evals": ne.value, "total_ms": tm.value}

    def set_profile_kernels(self, on: bool):
        abi.check(self.lib, self.lib.koordhip_set_profile_kernels(self._ctx, 1 if on else 0))

    def kernel_stats(self) -> dict:
        """Per-kernel device time of the last place call (profile_kernels=True)."""
        st = abi.KoordhipKernelStats()
        abi.check(self.lib, self.lib.koordhip_last_kernel_stats(self._ctx, C.byref(st)))
        return {f: getattr(st, f) for f, _ in abi.KoordhipKernelStats._fields_ if f != "reserved"}

    def kernel_names(self) -> dict:
        """Template instantiations of the last place call's evaluation and
        resolve launches, spelled as rocprofv3 names them."""
        ev, rs = C.create_string_buffer(64), C.create_string_buffer(64)
        abi.check(self.lib, self.lib.koordhip_last_kernel_names(self._ctx, ev, rs, 64))
        return {"eval": ev.value.decode(), "resolve": rs.value.decode()}

    # ---- multi-GPU ----------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = abi.load_library()
        buf = C.create_string_buffer(abi.UNIQUE_ID_BYTES)
        abi.check(lib, lib.koordhip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, world: int, rank: int):
        abi.check(self.lib, self.lib.koordhip_comm_init(self._ctx, uid, world, rank))

    @staticmethod
    def comm_init_local(engines):
        """One process, several contexts (GPUs, or contexts sharing one GPU):
        engines[r] becomes rank r of a node-sharded group (koordhip_comm_init_local)."""
        lib = abi.load_library()
        arr = (C.c_void_p * len(engines))(*[e._ctx.value for e in engines])
        abi.check(lib, lib.koordhip_comm_init_local(arr, len(engines)))


def place_stream_group(engines, pods: np.ndarray) -> list:
    """Collective place_stream over a local group: one host thread per context
    (ctypes releases the GIL for the duration of each call)."""
    import threading
    out = [None] * len(engines)
    err = [None] * len(engines)

    def run(r):
        try:
            out[r] = engines[r].place_stream(pods)
        except Exception as e:  # noqa: BLE001 - re-raised below
            err[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(len(engines))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return out
