// Stand-alone check of the place call's decisions
// (koordinator_amd/csrc/place_plan.hpp: plan_place, a pure function of the
// context's facts and the KOORDHIP_* knobs): hand-worked rows, then invariants
// over a grid of knobs and shapes.  tests/test_place_plan.py builds it with the
// host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>

#include "../koordinator_amd/csrc/place_plan.hpp"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {

using kh::PlaceFacts;
using kh::PlaceKnobs;
using kh::PlacePlan;
using kh::plan_place;

// the header's constants, as the tables below read them
static_assert(kh::kResolveMaxK == 128 && kh::kMaxBatch == 64 && kh::kClsTarget == 2048 && kh::kClsLead == 12, "rows");
constexpr int32_t kAmaxMin = 4 * kh::kClsLead + 2;  // 50

// LDS stubs: one that always fits, one linear in P, one that never fits
int32_t lds_fits(int32_t, int32_t, int32_t, int, int32_t) { return 0; }
constexpr int32_t kPerPod = 8192;  // 157 KiB / 8 KiB: 19 pods fit, 20 do not
int32_t lds_linear(int32_t P, int32_t, int32_t, int, int32_t) { return P * kPerPod; }
int32_t lds_never(int32_t, int32_t, int32_t, int, int32_t) { return 1 << 30; }
size_t cls_fits(int32_t, int32_t) { return 0; }
size_t cls_too_large(int32_t, int32_t) { return kh::kClsLdsBudget + 1; }

// a lone context, no side rows, few classes
PlaceFacts lone(int32_t batch) {
  PlaceFacts f;
  f.n = 5000;
  f.batch = batch;
  f.n_staged = 1000;
  f.n_cu = 256;
  f.nbins = 202;
  f.n_classes = 8;
  f.resolve_lds_bytes = lds_fits;
  f.cls_run_lds = cls_fits;
  return f;
}

// a rank of a two-GPU node-sharded job
PlaceFacts sharded() {
  PlaceFacts f = lone(24);
  f.world = 2;
  f.has_comm = f.has_comm2 = true;
  return f;
}

// a batch with device pods that the pipeline takes
PlaceFacts device_batch() {
  PlaceFacts f = lone(24);
  f.seq_profile = f.seq_ext_only = f.staged_ext = f.staged_ext_dev = f.podx_staged = true;
  f.n_ext = 40;
  return f;
}

int32_t amax(const PlacePlan &p) { return (kh::kClsTarget - p.K) / p.P; }

void hand_worked() {
  const PlaceKnobs none;
  {  // batch -> lag, K, amax, cls
    const struct { int32_t batch, lag, K, amax; bool cls; } rows[] = {
        {24, 2, 72, 82, true}, {32, 2, 96, 61, true}, {40, 1, 80, 49, false}, {64, 1, 128, 30, false}};
    for (const auto &r : rows) {
      const PlacePlan p = plan_place(lone(r.batch), none);
      CHECK(!p.seq && !p.err && p.P == r.batch && p.lag == r.lag && p.K == r.K && amax(p) == r.amax && p.cls == r.cls);
      CHECK(p.two && p.persistent && !p.serial && !p.local && !p.exch && !p.ext_pipe);
      CHECK(p.rounds == (1000 + r.batch - 1) / r.batch && p.lead == p.lag && p.tstride == 1);
    }
  }
  {  // side rows and the lag
    PlaceFacts f = lone(16);
    f.side = true;
    f.side_mode = 1;
    PlaceKnobs k;
    CHECK(plan_place(f, k).lag == 1);
    k.LAG2 = true;
    CHECK(plan_place(f, k).lag == 2);
    k.LAG1 = true;
    CHECK(plan_place(f, k).lag == 1);
    k = PlaceKnobs{};
    f.resv = true;
    f.side_mode = 3;
    CHECK(plan_place(f, k).lag == 2);
    k.LAG1 = true;
    CHECK(plan_place(f, k).lag == 1);
    CHECK(plan_place(lone(24), k).lag == 1);
  }
  {  // whatever takes the second evaluation stream away: lag 1, no class lists
    PlaceKnobs k[3];
    k[0].SERIAL = k[1].ROUND_LAUNCH = k[2].ONE_EVAL_STREAM = true;
    for (const PlaceKnobs &q : k) {
      const PlacePlan p = plan_place(lone(24), q);
      CHECK(!p.two && p.lag == 1 && p.K == 48 && !p.cls);
    }
    CHECK(plan_place(lone(24), k[0]).serial && !plan_place(lone(24), k[0]).persistent);
    CHECK(!plan_place(lone(24), k[1]).serial && !plan_place(lone(24), k[1]).persistent);
    CHECK(plan_place(lone(24), k[2]).persistent);
    PlaceFacts g = lone(24);
    g.has_group = true;
    g.world = 2;
    PlacePlan p = plan_place(g, none);
    CHECK(!p.two && !p.persistent && p.lag == 1 && !p.cls && p.exch && !p.local);
  }
  {  // the class lists' own conditions
    PlaceKnobs k;
    k.CLS_OFF = true;
    CHECK(!plan_place(lone(24), k).cls && plan_place(lone(24), k).lag == 2);
    PlaceFacts f = lone(24);
    f.n_classes = 0;
    CHECK(!plan_place(f, none).cls);
    f = lone(24);
    f.n_classes = 129;  // > n_cu / 2
    CHECK(!plan_place(f, none).cls);
    f.n_classes = 128;
    CHECK(plan_place(f, none).cls);
    f.nbins = 32769;
    CHECK(!plan_place(f, none).cls);
    f = lone(24);
    f.cls_run_lds = cls_too_large;
    CHECK(!plan_place(f, none).cls);
  }
  {  // node-sharded ranks
    PlacePlan p = plan_place(sharded(), none);
    CHECK(p.local && !p.exch && p.two && p.cls && p.lag == 2);
    PlaceKnobs k;
    k.SHARD_FORCE = true;
    p = plan_place(sharded(), k);
    CHECK(!p.local && p.exch && p.two && !p.cls && p.lag == 2);
    PlaceFacts f = sharded();
    f.n_classes = 129;
    p = plan_place(f, none);
    CHECK(!p.local && p.exch && p.two && !p.cls);
    f.has_comm2 = false;
    p = plan_place(f, none);
    CHECK(!p.local && p.exch && !p.two && p.lag == 1 && !p.cls);
    // a one-rank communicator: the exchange path on one GPU
    f = lone(24);
    f.has_comm = f.has_comm2 = true;
    p = plan_place(f, none);
    CHECK(!p.local && p.exch && p.two && !p.cls && p.lag == 2);
    k = PlaceKnobs{};
    k.SHARD_LOCAL_SIM = true;
    CHECK(!plan_place(f, k).local);  // (the knob is a lone context's)
    p = plan_place(lone(24), k);
    CHECK(p.local && !p.exch && p.two && p.cls);
  }
  {  // device pods inside the pipeline: every conjunct once
    const PlacePlan p = plan_place(device_batch(), none);
    CHECK(p.ext_pipe && !p.seq && p.cls && p.lag == 2 && p.lead == 2);
    bool PlaceFacts::*const need[] = {&PlaceFacts::seq_profile, &PlaceFacts::seq_ext_only, &PlaceFacts::staged_ext,
                                      &PlaceFacts::staged_ext_dev, &PlaceFacts::podx_staged};
    for (auto m : need) {
      PlaceFacts f = device_batch();
      f.*m = false;
      const PlacePlan q = plan_place(f, none);
      // (without the profile nothing asks for the sequential cycle -- the driver refuses such records;
      // without ext content the batch is an ordinary one)
      const bool seq = m != &PlaceFacts::seq_profile && m != &PlaceFacts::staged_ext;
      CHECK(!q.ext_pipe && q.seq == seq);
    }
    bool PlaceFacts::*const bar[] = {&PlaceFacts::staged_reserve, &PlaceFacts::seq_snap, &PlaceFacts::resv_dev_slot,
                                     &PlaceFacts::has_comm, &PlaceFacts::has_group};
    for (auto m : bar) {
      PlaceFacts f = device_batch();
      f.*m = true;
      const PlacePlan q = plan_place(f, none);
      CHECK(!q.ext_pipe && q.seq && q.lag == 0 && q.P == 1 && q.rounds == 1000);
    }
    PlaceFacts f = device_batch();
    f.side_mode = 1;
    CHECK(!plan_place(f, none).ext_pipe && plan_place(f, none).seq);
    f = device_batch();
    f.world = 2;
    CHECK(!plan_place(f, none).ext_pipe && plan_place(f, none).seq);
    PlaceKnobs k[3];
    k[0].SERIAL = k[1].ROUND_LAUNCH = k[2].EXT_SEQ = true;
    for (const PlaceKnobs &q : k) CHECK(!plan_place(device_batch(), q).ext_pipe && plan_place(device_batch(), q).seq);
    // the lead is never below the lag
    PlaceKnobs l;
    l.EXT_LEAD = 1;
    CHECK(plan_place(device_batch(), l).lead == 2);
    l.EXT_LEAD = 5;
    CHECK(plan_place(device_batch(), l).lead == 5);
    l.LAG1 = true;
    l.EXT_LEAD = 0;
    CHECK(plan_place(device_batch(), l).lead == 1);
  }
  {  // the resolve's LDS lowers the round
    PlaceFacts f = lone(24);
    f.resolve_lds_bytes = lds_linear;
    PlacePlan p = plan_place(f, none);
    CHECK(!p.err && p.lag == 2 && p.P == 19 && p.K == 57 && p.rounds == 53);  // the lag is chosen for batch_pods
    f.batch = 19;
    CHECK(plan_place(f, none).P == 19);
    f.resolve_lds_bytes = lds_never;
    p = plan_place(f, none);
    CHECK(p.err && p.msg && p.P == 1);
  }
  {  // the persistent resolve's monotone argument
    PlaceFacts f = lone(24);
    PlaceKnobs k;
    CHECK(plan_place(f, k).mono == 7);
    k.CHAIN_OFF = true;
    CHECK(plan_place(f, k).mono == 5);
    const int32_t want[4] = {3, 7, 11, 15};
    for (int32_t cp = 0; cp < 4; cp++) {
      k = PlaceKnobs{};
      k.CHAIN_PASSES = cp;
      CHECK(plan_place(f, k).mono == want[cp]);
      f.monotone = 0;
      CHECK(plan_place(f, k).mono == 0);
      k.CHAIN_OFF = true;
      CHECK(plan_place(f, k).mono == 0);
      f.monotone = 1;
    }
  }
}

void grid() {
  bool PlaceKnobs::*const flags[] = {
      &PlaceKnobs::SERIAL,  &PlaceKnobs::ROUND_LAUNCH,    &PlaceKnobs::ONE_EVAL_STREAM, &PlaceKnobs::CLS_OFF,
      &PlaceKnobs::SHARD_LOCAL_SIM, &PlaceKnobs::SHARD_FORCE, &PlaceKnobs::LAG1,        &PlaceKnobs::LAG2,
      &PlaceKnobs::EXT_SEQ, &PlaceKnobs::CHAIN_OFF,       &PlaceKnobs::STAMPS};
  const int nf = (int)(sizeof(flags) / sizeof(flags[0]));
  const int32_t batches[] = {1, 15, 16, 24, 32, 40, 64};
  long points = 0;
  for (unsigned mask = 0; mask < (1u << nf); mask++) {
    PlaceKnobs k;
    for (int b = 0; b < nf; b++) k.*flags[b] = (mask >> b) & 1;
    for (int32_t batch : batches)
      for (int32_t world = 1; world <= 2; world++)
        for (int sr = 0; sr < 4; sr++)
          for (int comm2 = 0; comm2 < world; comm2++) {
            PlaceFacts f = lone(batch);
            f.world = world;
            f.has_comm = world > 1;
            f.has_comm2 = comm2 != 0;
            f.side = (sr & 1) != 0;
            f.resv = (sr & 2) != 0;
            f.side_mode = f.resv ? 3 : f.side ? 1 : 0;
            f.n_staged = 1000 + batch;
            const PlacePlan p = plan_place(f, k);
            points++;
            CHECK(!p.seq && !p.err);
            CHECK((p.lag == 1 || p.lag == 2) && p.K == (p.lag + 1) * p.P && p.P == batch);
            if (p.lag == 2) CHECK(3 * p.P <= kh::kResolveMaxK && 2 * p.P <= kh::kMaxBatch && p.two);
            if (p.cls) CHECK(p.two && !p.exch && amax(p) >= kAmaxMin);
            if (p.local) CHECK(!p.exch);
            if (p.ext_pipe) CHECK(!p.seq);
            CHECK(p.rounds == (f.n_staged + p.P - 1) / p.P && (int64_t)p.rounds * p.P >= f.n_staged &&
                  (int64_t)(p.rounds - 1) * p.P < f.n_staged);
          }
  }
  CHECK(points == (1l << nf) * 7 * 3 * 4);
  // device batches: ext_pipe and seq exclude each other under every knob
  for (unsigned mask = 0; mask < (1u << nf); mask++) {
    PlaceKnobs k;
    for (int b = 0; b < nf; b++) k.*flags[b] = (mask >> b) & 1;
    const PlacePlan p = plan_place(device_batch(), k);
    CHECK(p.ext_pipe != p.seq);
    if (p.seq) CHECK(p.lag == 0 && p.P == 1 && !p.cls && !p.local);
  }
}

}  // namespace

int main() {
  hand_worked();
  grid();
  std::printf("place_plan_check ok\n");
  return 0;
}
