// modopti_online_host_check.cpp -- a stand-alone host program around the on-line half of aomarl_modopti_host.h (the
// per-frame schedule of aomarl_modopti_online_push / aomarl_do_control and the desc validation of
// aomarl_modopti_online_create), meant to be built with the address and undefined-behaviour sanitizers:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o modopti_online_host_check modopti_online_host_check.cpp
// No GPU, no HIP.  The schedule is run against a frame-by-frame model that has no ring: every frame must be consumed
// exactly once, in order, with the since-restart index the model gives it, before any apply that has to see it; applies
// fall where the statement puts them; restarts in the middle of a ring lose nothing.  The validator is fed every
// malformed desc it is written to refuse.  Exit status 0: all held.
#include "aomarl_modopti_host.h"
#include <stdlib.h>
#include <vector>

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) { fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

// frames the bank has consumed so far: (index since restart) of each, in order
struct Consumed { std::vector<long long> idx; };

static int take(Consumed &cs, std::vector<long long> &ring, const MoAction &a, int chunk) {
  if (a.flush == 0) return 0;
  REQUIRE(a.flush >= 1 && a.flush <= chunk && (size_t)a.flush == ring.size());
  for (int r = 0; r < a.flush; r++) {
    REQUIRE(ring[r] == a.t0 + r);          // row r of the ring is frame t0 + r since the restart
    cs.idx.push_back(ring[r]);
  }
  ring.clear();
  return 0;
}

static int run_schedule(int chunk, long long period, long long nskip, int nframes, int restart_every) {
  MoSchedule s;
  s.chunk = chunk; s.period = period; s.nskip = nskip;
  Consumed cs;
  std::vector<long long> ring;               // what the device ring holds: the since-restart index of each waiting row
  std::vector<long long> want;               // the model: since-restart index of every frame pushed
  long long since = 0, counted = 0, updates = 0;
  for (int t = 0; t < nframes; t++) {
    if (restart_every && t && t % restart_every == 0) {
      REQUIRE(take(cs, ring, mo_online_drain(s), chunk) == 0);
      mo_online_restart(s);
      since = 0;
      REQUIRE(s.fill == 0 && s.since == 0);
    }
    // the model
    want.push_back(since);
    if (since >= nskip) counted++;
    since++;
    const bool apply = (t + 1) % period == 0 && counted > 0;
    if (apply) updates++;
    // the schedule
    const MoAction a = mo_online_step(s);
    REQUIRE(a.slot == (int)ring.size() && a.slot < chunk);
    ring.push_back(want.back());
    REQUIRE(a.apply == apply);
    REQUIRE(take(cs, ring, a, chunk) == 0);
    if (apply) REQUIRE(cs.idx.size() == want.size());         // the apply sees every frame pushed so far
    REQUIRE((int)ring.size() == s.fill && s.fill < chunk);    // a full ring never waits
    REQUIRE(s.total == t + 1 && s.since == since && s.counted == counted && s.updates == updates);
  }
  REQUIRE(take(cs, ring, mo_online_drain(s), chunk) == 0);
  REQUIRE(cs.idx == want);
  return 0;
}

int main() {
  const int chunks[] = {1, 2, 7, 31, 32};
  const long long periods[] = {1, 5, 31, 32, 33, 256};
  const long long nskips[] = {0, 1, 40, 1000};
  const int restarts[] = {0, 1, 13, 64, 100};
  for (int c : chunks) for (long long p : periods) for (long long k : nskips) for (int r : restarts)
    REQUIRE(run_schedule(c, p, k, 300, r) == 0);
  // nskip beyond every episode: nothing ever enters J, nothing is ever applied
  { MoSchedule s; s.chunk = 4; s.period = 3; s.nskip = 50;
    for (int t = 0; t < 200; t++) { if (t % 40 == 0) { mo_online_drain(s); mo_online_restart(s); } REQUIRE(!mo_online_step(s).apply); }
    REQUIRE(s.updates == 0 && s.counted == 0); }
  // counted is sticky across a restart: J is kept, so applies go on during the next episode's transient
  { MoSchedule s; s.chunk = 32; s.period = 10; s.nskip = 15;
    for (int t = 0; t < 20; t++) mo_online_step(s);
    REQUIRE(s.updates == 1);
    mo_online_drain(s); mo_online_restart(s);
    for (int t = 0; t < 10; t++) mo_online_step(s);
    REQUIRE(s.updates == 2 && s.counted == 5); }

  // ---- the validator
  std::string err;
  const float g[3] = {0.f, 0.3f, 0.6f};
  const double G0[8] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8};
  aomarl_modopti_online_desc ok;
  ok.nenv = 2; ok.nmodes = 4; ok.ngain = 3; ok.nskip = 5; ok.chunk = 32; ok.period = 256; ok.pool = 1;
  ok.delay = 1.f; ok.forget = 1.0; ok.beta = 1.0; ok.gains = g; ok.G0 = nullptr;
  REQUIRE(mo_online_validate(&ok, err) == 0);
  REQUIRE(mo_online_validate(nullptr, err) == 1 && err.find("null desc") != std::string::npos);
  { auto d = ok; d.G0 = G0; REQUIRE(mo_online_validate(&d, err) == 0); }
  { auto d = ok; d.G0 = G0; d.pool = 0; REQUIRE(mo_online_validate(&d, err) == 0); }        // reads all 2 x 4
  { auto d = ok; d.nenv = 0; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("modopti_online_create: nenv") == 0); }
  { auto d = ok; d.nmodes = 0; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("nmodes") != std::string::npos); }
  { auto d = ok; d.ngain = 0; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("ngain") != std::string::npos); }
  { auto d = ok; d.gains = nullptr; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("null gains") != std::string::npos); }
  { auto d = ok; d.nskip = -1; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("nskip") != std::string::npos); }
  { auto d = ok; d.delay = 2.5f; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("delay") != std::string::npos); }
  for (int c : {0, -1, 33}) { auto d = ok; d.chunk = c; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("chunk") != std::string::npos); }
  for (int c : {1, 32}) { auto d = ok; d.chunk = c; REQUIRE(mo_online_validate(&d, err) == 0); }
  for (int p : {0, -3}) { auto d = ok; d.period = p; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("period") != std::string::npos); }
  for (int p : {2, -1}) { auto d = ok; d.pool = p; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("pool") != std::string::npos); }
  for (double f : {0.0, -0.5, 1.0000001, (double)NAN, (double)INFINITY}) {
    auto d = ok; d.forget = f; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("forget") != std::string::npos);
    auto b = ok; b.beta = f; REQUIRE(mo_online_validate(&b, err) == 1 && err.find("beta") != std::string::npos);
  }
  for (double f : {1e-6, 0.5, 1.0}) { auto d = ok; d.forget = f; d.beta = f; REQUIRE(mo_online_validate(&d, err) == 0); }
  { const float bad[2] = {1.f, 1.5f}; auto d = ok; d.ngain = 2; d.gains = bad;               // delay 1: stable iff g < 1
    REQUIRE(mo_online_validate(&d, err) == 1 && err.find("stable") != std::string::npos); }
  { double g0[4] = {0.1, NAN, 0.1, 0.1}; auto d = ok; d.G0 = g0; REQUIRE(mo_online_validate(&d, err) == 1 && err.find("G0[1]") != std::string::npos); }
  printf("modopti_online_host_check: ok\n");
  return 0;
}
