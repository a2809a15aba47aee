// timers_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_timers.h and the seven
// wgcs_timers_*_host forms of timers.cpp, the code the lanes of timers_kernels.hip run, as plain host
// code (built by tests/test_timers_host.py with -fsanitize=address,undefined together with timers.cpp).
//
// Every table is copied into a heap buffer of exactly its size, and every output is a heap
// buffer of exactly its size, so a read or a write past either end is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = absent: a NULL pointer, no rows); scalars are little-endian:
//   sent <row|host> <sizes: 4 B each> <peer: 4 B each> <count: 4 B each> <status: 4 B each> <job_key: 4 B each>
//        <max_segs: 4 B> <now: 8 B> <seed: 4 B> <peer_rows: 4 B each> <timers: 64 B each>        -> timers
//   rcvd <row|host> <groups: 24 B each> <calls_per_batch: 4 B> <now> <peer_rows> <timers>        -> timers
//   init <row|host> <reasons: 4 B each> <start_peer: 4 B each> <init_status: 4 B each> <now> <seed> <timers>
//                                                                                                -> timers
//   resp <row|host> <resp: 80 B each> <gate: 4 B each> <now> <timers>                            -> timers
//   fin  <row|host> <arena> <pkts: 24 B each> <gate> <begun: 4 B each> <now> <hs_slots: 8 B each>
//        <states: 128 B each> <timers> <rekey: 16 B each>                                        -> timers | rekey
//   rot  <row|host> <pkts> <rotated: 4 B each> <now> <key_peer: 4 B each> <peer_rows> <timers> <rekey>
//                                                                                                -> timers | rekey
//   exp  <row|host> <now> <timers> <rekey> <table: 72 B each> <staged: 4 B each> <kp: 80 B each> <slots>
//        <peer_keys: 8 B each> <keys: 48 B each> <key_peer> <n_ka_max: 4 B>
//        -> ka_peer | ka_count | ka_sizes | ka_status | n_ka | actions | timers | rekey | kp | slots | peer_keys |
//           keys | key_peer
// "row" calls the row functions in the order of the host form, "host" the host form itself.
// An output starts as 0xEE.  stdout: one line per call, then "timers_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_timers.h"

using namespace wgcs;

// a heap copy of exactly the bytes given, aligned as operator new aligns; p stays NULL for none
struct Exact {
  std::unique_ptr<uint8_t[]> mem;
  uint8_t* p = nullptr;
  size_t n = 0;
  Exact(const std::vector<uint8_t>& v) : n(v.size()) {
    if (n == 0) return;
    mem.reset(new uint8_t[n]);
    p = mem.get();
    memcpy(p, v.data(), n);
  }
};

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static void print_hex(const Exact& e) {
  if (e.n == 0) printf("-");
  for (size_t i = 0; i < e.n; ++i) printf("%02x", e.p[i]);
}

static std::vector<uint8_t> filled(size_t n) { return std::vector<uint8_t>(n, 0xEE); }

// the tests run on little-endian hosts, as the library's layouts assume
template <typename T>
static bool scalar(const std::vector<uint8_t>& f, T* out) {
  if (f.size() != sizeof(T)) return false;
  memcpy(out, f.data(), sizeof(T));
  return true;
}

// a body of the header for every entry in order, as the host forms run it
template <class F>
static void each(const F& f, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) f(i);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, how;
    if (!(in >> op >> how) || (how != "row" && how != "host")) return 2;
    const bool host = how == "host";
    std::vector<std::vector<uint8_t>> f;
    for (std::string t; in >> t;) f.push_back(unhex(t));
    std::vector<const Exact*> outs;
    std::vector<std::unique_ptr<Exact>> keep;
    auto exact = [&](const std::vector<uint8_t>& v) {
      keep.emplace_back(new Exact(v));
      return keep.back().get();
    };
    int64_t now = 0;
    uint32_t seed = 0;
    if (op == "sent") {
      uint32_t max_segs = 0;
      if (f.size() != 10 || f[2].size() % 4 || f[3].size() != f[2].size() || f[4].size() != f[2].size() ||
          !scalar(f[5], &max_segs) || f[0].size() != f[2].size() * max_segs || f[1].size() != f[0].size() ||
          !scalar(f[6], &now) || !scalar(f[7], &seed) || f[8].size() % 4 || f[9].size() % sizeof(wgcs_timers))
        return 2;
      const Exact *sizes = exact(f[0]), *peer = exact(f[1]), *count = exact(f[2]), *status = exact(f[3]);
      const Exact *job_key = exact(f[4]), *rows = exact(f[8]), *timers = exact(f[9]);
      const uint32_t n = (uint32_t)(count->n / 4), n_ids = (uint32_t)(rows->n / 4);
      const uint32_t n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      const auto* const sz = (const int32_t*)sizes->p;
      const auto* const pe = (const uint32_t*)peer->p;
      const auto* const c = (const int32_t*)count->p;
      const auto* const st = (const int32_t*)status->p;
      const auto* const jk = (const uint32_t*)job_key->p;
      const auto* const pr = (const uint32_t*)rows->p;
      auto* const tm = (wgcs_timers*)timers->p;
      if (host) {
        if (wgcs_timers_sent_host(sz, pe, c, st, jk, n, max_segs, now, seed, pr, n_ids, tm, n_peers) != 0) return 3;
      } else {
        each(TimersSent{{{pe, c, st, max_segs, pr, n_ids, n_peers}, jk}, sz, now, seed, tm}, n);
      }
      outs = {timers};
    } else if (op == "rcvd") {
      uint32_t cpb = 0;
      if (f.size() != 5 || f[0].size() % sizeof(wgcs_write_group) || !scalar(f[1], &cpb) || cpb == 0 ||
          !scalar(f[2], &now) || f[3].size() % 4 || f[4].size() % sizeof(wgcs_timers))
        return 2;
      const Exact *groups = exact(f[0]), *rows = exact(f[3]), *timers = exact(f[4]);
      const uint32_t n = (uint32_t)(groups->n / sizeof(wgcs_write_group)), n_ids = (uint32_t)(rows->n / 4);
      const uint32_t n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      if (n % cpb) return 2;
      const auto* const g = (const wgcs_write_group*)groups->p;
      const auto* const pr = (const uint32_t*)rows->p;
      auto* const tm = (wgcs_timers*)timers->p;
      if (host) {
        if (wgcs_timers_received_host(g, n / cpb, cpb, now, pr, n_ids, tm, n_peers) != 0) return 3;
      } else {
        each(TimersReceived{{g, pr, n_ids, n_peers}, now, tm}, n);
      }
      outs = {timers};
    } else if (op == "init") {
      if (f.size() != 6 || f[1].size() % 4 || f[2].size() != f[1].size() || !scalar(f[3], &now) ||
          !scalar(f[4], &seed) || f[5].size() % sizeof(wgcs_timers) ||
          f[0].size() != f[5].size() / sizeof(wgcs_timers) * 4)
        return 2;
      const Exact *reasons = exact(f[0]), *start_peer = exact(f[1]), *status = exact(f[2]), *timers = exact(f[5]);
      const uint32_t n_tickets = (uint32_t)(start_peer->n / 4), n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      const auto* const why = (const uint32_t*)reasons->p;
      const auto* const sp = (const uint32_t*)start_peer->p;
      const auto* const st = (const int32_t*)status->p;
      auto* const tm = (wgcs_timers*)timers->p;
      if (host) {
        if (wgcs_timers_initiated_host(why, sp, st, n_tickets, now, seed, tm, n_peers) != 0) return 3;
      } else {
        each(TimersFresh{why, tm}, n_peers);
        each(TimersInitiated{{sp, st, n_peers}, now, seed, tm}, n_tickets);
      }
      outs = {timers};
    } else if (op == "resp") {
      if (f.size() != 4 || f[0].size() % sizeof(wgcs_hs_resp) || f[1].size() != f[0].size() / sizeof(wgcs_hs_resp) * 4 ||
          !scalar(f[2], &now) || f[3].size() % sizeof(wgcs_timers))
        return 2;
      const Exact *resp = exact(f[0]), *gate = exact(f[1]), *timers = exact(f[3]);
      const uint32_t n = (uint32_t)(resp->n / sizeof(wgcs_hs_resp)), n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      const auto* const r = (const wgcs_hs_resp*)resp->p;
      const auto* const g = (const int32_t*)gate->p;
      auto* const tm = (wgcs_timers*)timers->p;
      if (host) {
        if (wgcs_timers_responded_host(r, g, n, now, tm, n_peers) != 0) return 3;
      } else {
        each(TimersResponded{{r, g, n_peers}, now, tm}, n);
      }
      outs = {timers};
    } else if (op == "fin") {
      if (f.size() != 9 || f[1].size() % sizeof(wgcs_aead_pkt) || f[2].size() != f[1].size() / sizeof(wgcs_aead_pkt) * 4 ||
          f[3].size() != f[2].size() || !scalar(f[4], &now) || f[5].size() % sizeof(wgcs_session_slot) ||
          f[6].size() % sizeof(wgcs_hs_state) || f[7].size() % sizeof(wgcs_timers) ||
          f[8].size() != f[7].size() / sizeof(wgcs_timers) * sizeof(wgcs_rekey))
        return 2;
      const Exact *arena = exact(f[0]), *pkts = exact(f[1]), *gate = exact(f[2]), *begun = exact(f[3]);
      const Exact *hs_slots = exact(f[5]), *states = exact(f[6]), *timers = exact(f[7]), *rekey = exact(f[8]);
      const uint32_t n = (uint32_t)(pkts->n / sizeof(wgcs_aead_pkt));
      const uint32_t n_hs = (uint32_t)(hs_slots->n / sizeof(wgcs_session_slot));
      const uint32_t n_states = (uint32_t)(states->n / sizeof(wgcs_hs_state));
      const uint32_t n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      const auto* const pk = (const wgcs_aead_pkt*)pkts->p;
      const auto* const g = (const int32_t*)gate->p;
      const auto* const b = (const int32_t*)begun->p;
      const auto* const hs = (const wgcs_session_slot*)hs_slots->p;
      const auto* const st = (const wgcs_hs_state*)states->p;
      auto* const tm = (wgcs_timers*)timers->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      if (host) {
        if (wgcs_timers_finished_host(arena->p, pk, g, b, n, now, hs, n_hs, st, n_states, tm, rk, n_peers) != 0) return 3;
      } else {
        each(TimersFinished{{arena->p, pk, g, hs, n_hs, st, n_states, n_peers}, b, now, tm, rk}, n);
      }
      outs = {timers, rekey};
    } else if (op == "rot") {
      if (f.size() != 7 || f[0].size() % sizeof(wgcs_aead_pkt) || f[1].size() != f[0].size() / sizeof(wgcs_aead_pkt) * 4 ||
          !scalar(f[2], &now) || f[3].size() % 4 || f[4].size() % 4 || f[5].size() % sizeof(wgcs_timers) ||
          f[6].size() != f[5].size() / sizeof(wgcs_timers) * sizeof(wgcs_rekey))
        return 2;
      const Exact *pkts = exact(f[0]), *rotated = exact(f[1]), *key_peer = exact(f[3]), *rows = exact(f[4]);
      const Exact *timers = exact(f[5]), *rekey = exact(f[6]);
      const uint32_t n = (uint32_t)(pkts->n / sizeof(wgcs_aead_pkt)), n_keys = (uint32_t)(key_peer->n / 4);
      const uint32_t n_ids = (uint32_t)(rows->n / 4), n_peers = (uint32_t)(timers->n / sizeof(wgcs_timers));
      const auto* const pk = (const wgcs_aead_pkt*)pkts->p;
      const auto* const ro = (const uint32_t*)rotated->p;
      const auto* const kpr = (const uint32_t*)key_peer->p;
      const auto* const pr = (const uint32_t*)rows->p;
      auto* const tm = (wgcs_timers*)timers->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      if (host) {
        if (wgcs_timers_rotated_host(pk, ro, n, now, kpr, n_keys, pr, n_ids, tm, rk, n_peers) != 0) return 3;
      } else {
        each(TimersRotated{{pk, kpr, n_keys, pr, n_ids, n_peers}, ro, now, tm, rk}, n);
      }
      outs = {timers, rekey};
    } else if (op == "exp") {
      uint32_t room = 0;
      if (f.size() != 11 || !scalar(f[0], &now) || f[1].size() % sizeof(wgcs_timers)) return 2;
      const size_t np = f[1].size() / sizeof(wgcs_timers);
      if (f[2].size() != np * sizeof(wgcs_rekey) || f[3].size() != np * sizeof(wgcs_peer_key) ||
          (f[4].size() != 0 && f[4].size() != np * 4) || f[5].size() != np * sizeof(wgcs_keypairs) ||
          f[6].size() % sizeof(wgcs_session_slot) || f[7].size() % sizeof(wgcs_session_slot) ||
          f[8].size() % sizeof(wgcs_aead_key) || f[9].size() != f[8].size() / sizeof(wgcs_aead_key) * 4 ||
          !scalar(f[10], &room))
        return 2;
      const Exact *timers = exact(f[1]), *rekey = exact(f[2]), *table = exact(f[3]), *staged = exact(f[4]);
      const Exact *kp = exact(f[5]), *slots = exact(f[6]), *peer_keys = exact(f[7]), *keys = exact(f[8]);
      const Exact* const key_peer = exact(f[9]);
      const uint32_t n_peers = (uint32_t)np, n_slots = (uint32_t)(slots->n / sizeof(wgcs_session_slot));
      const uint32_t n_peer_slots = (uint32_t)(peer_keys->n / sizeof(wgcs_session_slot));
      const uint32_t n_keys = (uint32_t)(keys->n / sizeof(wgcs_aead_key));
      const Exact *ka_peer = exact(filled(4 * (size_t)room)), *ka_count = exact(filled(4 * (size_t)room));
      const Exact *ka_sizes = exact(filled(4 * (size_t)room)), *ka_status = exact(filled(4 * (size_t)room));
      const Exact *n_ka = exact(filled(4)), *actions = exact(filled(4 * np));
      auto* const tm = (wgcs_timers*)timers->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      const auto* const tb = (const wgcs_peer_key*)table->p;
      const auto* const sg = (const uint32_t*)staged->p;
      auto* const k = (wgcs_keypairs*)kp->p;
      auto* const sl = (wgcs_session_slot*)slots->p;
      auto* const pks = (wgcs_session_slot*)peer_keys->p;
      auto* const ks = (wgcs_aead_key*)keys->p;
      auto* const kpr = (uint32_t*)key_peer->p;
      auto* const kap = (uint32_t*)ka_peer->p;
      auto* const kac = (int32_t*)ka_count->p;
      auto* const kas = (int32_t*)ka_sizes->p;
      auto* const kat = (int32_t*)ka_status->p;
      auto* const cn = (uint32_t*)n_ka->p;
      auto* const act = (uint32_t*)actions->p;
      if (host) {
        if (wgcs_timers_expire_host(now, tm, rk, tb, n_peers, sg, k, sl, n_slots, pks, n_peer_slots, ks, kpr, n_keys, room,
                                    kap, kac, kas, kat, cn, act) != 0)
          return 3;
      } else {
        for (uint32_t r = 0; r < n_peers; ++r)
          timers_expire_verdict(r, now, tm, rk, tb, sg, k, sl, n_slots, pks, n_peer_slots, ks, kpr, n_keys, act);
        uint32_t rank = 0;
        for (uint32_t r = 0; r < n_peers; ++r)
          if (act[r] & WGCS_TIMERS_ACT_KEEPALIVE) timers_expire_commit(r, rank++, tm, tb, room, kap, kac, kas, kat, act);
        *cn = rank < room ? rank : room;
        for (uint32_t q = *cn; q < room; ++q) timers_expire_tail(q, kap, kac, kas, kat);
      }
      outs = {ka_peer, ka_count, ka_sizes, ka_status, n_ka, actions, timers, rekey, kp, slots, peer_keys, keys, key_peer};
    } else {
      return 2;
    }
    for (size_t i = 0; i < outs.size(); ++i) {
      if (i) printf(" ");
      print_hex(*outs[i]);
    }
    printf("\n");
  }
  printf("timers_host: ok\n");
  return 0;
}
