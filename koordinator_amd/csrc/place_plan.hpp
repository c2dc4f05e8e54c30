// place_plan.hpp -- the shape of one place call, decided once: which path it
// takes, its streams, its pipeline depth and its round size.  Host only: no
// HIP header, any C++17 compiler (tests/place_plan_check.cpp builds it alone).
//
// place_staged_impl (api.hip) reads the knobs, gathers the facts, calls
// plan_place and enqueues what the plan says; pmc_replay takes the same plan
// with the knobs cleared that take a call off the pipeline.  Every rule below
// is written here and nowhere else.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace kh {

constexpr int32_t kMaxBatch = 64;      // pods per round at most (the resolve's M' spans 2 rounds <= 2 x 64 slots)
constexpr int32_t kResolveMaxK = 128;  // longest list the resolve takes (RES_MAXP)
constexpr int32_t kClsTarget = 2048;   // keys a class build takes (the best ones, ties by lowest index)
constexpr int32_t kClsLead = 12;       // rounds a class build is enqueued ahead of its first use (cls_plan)
// Dynamic LDS the host plans for: the resolve's budget (below the kernel's own
// cap RES_LDS_MAX, kernels.hip) and the class workgroups' (k_cls_run).
constexpr int32_t kResolveLdsBudget = 157 * 1024;
constexpr size_t kClsLdsBudget = 150 * 1024;

// The log rounds a class build stays valid (api.hip cls_plan): each round can
// move at most P of its kClsTarget keys out of the valid range, and K must remain.
constexpr int32_t cls_amax(int32_t P, int32_t K) { return (kClsTarget - K) / P; }

// The KOORDHIP_* environment knobs of the place path, read
// at the start of every place call (api.hip read_place_knobs).
struct PlaceKnobs {
  bool SERIAL = false, ROUND_LAUNCH = false, ONE_EVAL_STREAM = false, CLS_OFF = false;
  bool SHARD_LOCAL_SIM = false, SHARD_FORCE = false, LAG1 = false, LAG2 = false;
  bool EXT_SEQ = false, CHAIN_OFF = false, STAMPS = false;
  bool SAMECLS_OFF = false;  // the resolve's same-class speculation off (A/B)
  bool NO_PRELOAD = false, NO_KEY_TABLES = false;  // the resolve's launcher (kernels.hip launch_resolve)
  int32_t EXT_LEAD = 0;       // unset: 0 (the lead is never below the lag)
  int32_t CHAIN_PASSES = 1;   // unset: 1
  int32_t TRACE_POD = -1;     // unset: -1 (no pod)
};

// What the decisions depend on, as plain values of the context.
struct PlaceFacts {
  int32_t n = 0, batch = 1, n_staged = 0, world = 1, n_cu = 256, nbins = 2, monotone = 1;
  int32_t n_classes = 0;  // pod classes of the staged batch (byte-identical device records)
  int32_t n_ext = 0;      // its device pods
  bool has_comm = false, has_comm2 = false, has_group = false;
  bool side = false, resv = false;
  int side_mode = 0;      // the kernels' node-row mode (kernels.h side_mode)
  bool seq_profile = false, seq_ext_only = false, seq_snap = false;
  bool staged_ext = false, staged_ext_dev = false, podx_staged = false, staged_reserve = false;
  bool resv_dev_slot = false;  // a reservation holds devices (DevNodes dv.rslot)
  // dynamic LDS of k_resolve for (P, K, n, side_mode, lag) and of k_cls_run for (n, monotone)
  int32_t (*resolve_lds_bytes)(int32_t, int32_t, int32_t, int, int32_t) = nullptr;
  size_t (*cls_run_lds)(int32_t, int32_t) = nullptr;
};

struct PlacePlan {
  bool seq = false;         // the sequential cycle places the batch (seq.hip); nothing below applies but P 1, lag 0
  bool ext_pipe = false;    // device pods inside the pipelined greedy
  bool serial = false;      // every launch on one stream, one resolve per round
  bool persistent = false;  // one resolve launch for the whole stream
  bool local = false;       // a node-sharded rank evaluates the full table itself
  bool exch = false;        // the rounds' lists are all-gathered and merged
  bool two = false;         // two evaluation streams, rounds alternating
  bool cls = false;         // class-incremental lists instead of per-round evaluations
  int32_t lag = 1, P = 1, K = 2, rounds = 0;
  int32_t lead = 1;         // device pods: rounds a pre-evaluation runs ahead of its hand-off
  int32_t mono = 0;         // the persistent resolve's monotone argument (bit 0 | chain bit 1 | passes bits 2-3 | same-class speculation off bit 4)
  int32_t tstride = 1;      // profile_kernels: every tstride-th round is timed
  int err = 0;              // nonzero: refuse the call with msg (an invalid argument)
  const char *msg = nullptr;
};

// Device pods among pods without ext content (DeviceShare as the only
// coupling plugin the records use, the plain plugin build, one GPU, the
// persistent pipeline): placed inside the pipelined greedy -- the resolve
// hands each one the exact state and k_ext_pre / k_ext_final run its reference cycle
// (seq.hip) -- instead of the whole batch in the sequential cycle.
// KOORDHIP_EXT_SEQ: the sequential cycle for such batches too (A/B).
inline bool ext_pipe_eligible(const PlaceFacts &f, const PlaceKnobs &k) {
  return f.seq_profile && f.seq_ext_only && f.staged_ext && f.staged_ext_dev && f.podx_staged && !f.staged_reserve &&
         !f.seq_snap && !f.resv_dev_slot && f.side_mode == 0 && f.world == 1 && !f.has_comm && !f.has_group &&
         !k.SERIAL && !k.ROUND_LAUNCH && !k.EXT_SEQ;
}

// class-incremental lists (cls.hip): the staged pods fall into few classes
// (byte-identical records); the second stream then runs the class builds
// (one persistent workgroup per class: every one resident, one per CU with
// half the CUs to spare for the resolve and the builds)
inline bool cls_eligible(const PlaceFacts &f, const PlaceKnobs &k) {
  return f.n_classes > 0 && f.nbins <= 32768 && !k.CLS_OFF && f.n_classes <= f.n_cu / 2 &&
         f.cls_run_lds(f.n, f.monotone) <= kClsLdsBudget;
}

// Pipeline depth: round r's lists are evaluated on the state after round
// r - 1 - lag.  Lag 2 (the default with the two evaluation streams) lets an
// evaluation overlap two resolve rounds; the resolve then re-evaluates the
// nodes of the last two rounds (k >= 3P).  Lag 1: k >= 2P.
// pods per round: batch_pods, lowered until the resolve kernel's LDS holds
// the round (NodeNUMAResource rows are large)
// (NodeNUMAResource streams are bound by the resolve's cpuset Reserve: the
// longer re-evaluated set of lag 2 measured slower there, 87k vs 93k pods/s
// (round 2), 149k vs 154k (round 3, config 3); the Reservation streams are
// bound by the evaluation -- the period of a round is (eval + resolve) / 2 at
// lag 1, / 3 at lag 2 -- and run lag 2: config 5 170k -> 182k pods/s in
// spite of the shorter rounds the resolve's LDS then allows (24 -> 15 pods).
// KOORDHIP_LAG2: lag 2 with NodeNUMAResource alone too.)
inline void round_shape(const PlaceFacts &f, const PlaceKnobs &k, PlacePlan *p) {
  int32_t P = f.batch;
  int32_t lag = (p->two && (!f.side || f.resv || k.LAG2) && !k.LAG1) ? 2 : 1;
  if (lag == 2 && (3 * P > kResolveMaxK || 2 * P > kMaxBatch)) lag = 1;  // M' spans 2 rounds <= 64 slots
  while (P > 1 && f.resolve_lds_bytes(P, (lag + 1) * P, f.n, f.side_mode, lag) > kResolveLdsBudget) P--;
  p->lag = lag;
  p->P = P;
  p->K = (lag + 1) * P;
  p->rounds = (f.n_staged + P - 1) / P;
}

// KOORDHIP_EXT_LEAD: the rounds between lag and lead add their commits, from
// the commit log, to a device pod's re-evaluated set
inline int32_t ext_lead(const PlaceKnobs &k, int32_t lag) { return std::max(lag, k.EXT_LEAD); }

inline PlacePlan plan_place(const PlaceFacts &f, const PlaceKnobs &k) {
  PlacePlan p;
  p.ext_pipe = ext_pipe_eligible(f, k);
  // the sequential cycle: a snapshot or profile that needs it, a reserve pod in
  // the batch, or an ext-record profile whose batch carries ext content.  An
  // empty record: DeviceShare's PreFilter skips the pod (Filter passes, Score 0,
  // no Reserve: deviceshare/plugin.go:162-182, scoring.go:33-40);
  // PodTopologySpread has no constraint (Filter passes; every Score 0, which
  // NormalizeScore turns into the same 100 on every node) and the pod counts
  // for none; InterPodAffinity has no term, no existing pod's term matches it
  // (Filter passes, Score 0 everywhere, normalised to 0) and it counts for no
  // entry -- nothing couples its nodes or changes the cycle's state.
  p.seq = f.staged_reserve || f.seq_snap || (f.seq_profile && (!f.seq_ext_only || f.staged_ext) && !p.ext_pipe);
  if (p.seq) {
    p.lag = 0, p.P = 1, p.K = 1, p.rounds = f.n_staged, p.lead = 0;
    return p;
  }
  // KOORDHIP_SERIAL (profiling under rocprofv3 --pmc, which serialises
  // dispatches): every launch on one stream in dependency order, one resolve
  // per round; the lists are then fresher than in the pipeline, which the
  // resolve treats exactly like refreshed entries.
  p.serial = k.SERIAL;
  p.persistent = !p.serial && !f.has_group && !k.ROUND_LAUNCH;
  // A lone single-GPU context alternates the rounds between two evaluation
  // streams (each with its own score matrix and select buffers; the resolve
  // counts finished lists per round parity).
  // exchanged: node-sharded, or a one-rank RCCL communicator (the exchange
  // path end to end on one GPU: all-gather, merge, per-round signal)
  // A node-sharded rank (world > 1) whose batch the class-incremental lists
  // cover evaluates the full table itself: every rank holds the full replica
  // and resolves every pod anyway, and sharding divides only the evaluation,
  // which the class lists already took off the critical path -- through the
  // per-round all-gather world > 1 would run slower than one GPU (DESIGN.md
  // section 6).  KOORDHIP_SHARD_FORCE keeps the exchange (A/B).
  const bool cls_fit = cls_eligible(f, k);
  // (KOORDHIP_SHARD_LOCAL_SIM: a lone one-GPU context takes that decision as
  // if it were a rank of a sharded job -- the path's one-GPU test)
  const bool local_sim = f.world == 1 && !f.has_comm && k.SHARD_LOCAL_SIM;
  p.local = (f.world > 1 || local_sim) && !f.has_group && p.persistent && cls_fit && !k.SHARD_FORCE;
  p.exch = (f.world > 1 || f.has_comm) && !p.local;
  // (node-sharded: the rounds of the second stream exchange on comm2)
  p.two = p.persistent && (!p.exch || f.has_comm2) && !k.ONE_EVAL_STREAM;
  round_shape(f, k, &p);
  // (builds are enqueued kClsLead rounds ahead and rebuilt amax / 2 rounds before they expire)
  p.cls = p.two && !p.exch && cls_fit && cls_amax(p.P, p.K) >= 4 * kClsLead + 2;
  p.lead = ext_lead(k, p.lag);
  // (monotone bit 1: the chained decisions, wave 0 at the start of each
  // round's loop: they take the staged-conflict pods off the general path --
  // config 4: 16.0k -> 0.4k general-path pods, 75.0 -> 62.5 ms per step,
  // profiles/r05n_chain_ab.txt; KOORDHIP_CHAIN_OFF for A/B)
  // (bits 2-3: chain passes, 1 by default -- 1 / 2 / 3 passes measured 60.1 /
  // 60.5 / 61.0 ms per step on config 4, r05o; KOORDHIP_CHAIN_PASSES for A/B.
  // With the final claim table built by the loop, r08a: 57.08-57.19 / 56.58-56.76 /
  // 57.11-57.23 ms, three lines each -- two passes win by 0.9 %, more than the
  // lines' spread; the default stays 1 until the plan's hand-worked rows move
  // with it, profiles/r08a_config4_ab.txt)
  // (bit 4, SET to turn it off so the default values above stay: the same-class
  // speculation of the prologue -- a round's pods of one class decided
  // together, k_resolve phase 1; KOORDHIP_SAMECLS_OFF for A/B)
  p.mono = f.monotone | ((f.monotone && !k.CHAIN_OFF) ? 2 : 0) | (f.monotone ? ((k.CHAIN_PASSES & 3) << 2) : 0) |
           ((f.monotone && k.SAMECLS_OFF) ? 16 : 0);
  // profile_kernels: event pairs around the evaluation launches of at most
  // ~256 evenly spaced rounds (the per-kernel averages need no more; every
  // outstanding timed event holds a runtime signal, and a host thread that
  // runs out of them waits for the oldest -- possibly behind the persistent
  // resolve, which waits for rounds that thread has not enqueued yet)
  p.tstride = std::max<int32_t>(1, (p.rounds + 255) / 256);
  if (f.resolve_lds_bytes(p.P, p.K, f.n, f.side_mode, p.lag) > kResolveLdsBudget) {
    p.err = 1;
    p.msg = "snapshot too large for the resolve kernel's LDS";
  }
  return p;
}

}  // namespace kh
