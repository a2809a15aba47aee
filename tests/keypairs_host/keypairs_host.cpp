// keypairs_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_keypairs.h
// (keypairs_begin, keypairs_received_claim, keypairs_received_commit, delete_session) and the host
// forms wgcs_keypairs_begin_responder_host / _begin_initiator_host / _received_host of keypairs.cpp,
// the code the lanes of keypairs_kernels.hip run, as plain host code (built by
// tests/test_keypairs_host.py with -fsanitize=address,undefined together with keypairs.cpp).
//
// Every table is copied into a heap buffer of exactly its size, and every output is a heap
// buffer of exactly its size, so a read or a write past either end is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = absent: a NULL pointer, no rows).  The tail of
// every line is the five tables the calls write:
//   <kp: 80 B each> <slots: 8 B each> <peer_keys: 8 B each> <keys: 48 B each> <key_peer: 4 B each>
//   resp <row|host> <resp: 80 B each> <gate: 4 B each> <now: 8 B LE> <table: 72 B each> tail
//   init <row|host> <arena> <pkts: 24 B each> <gate> <now> <hs_slots: 8 B each|-> <states: 128 B each|->
//        <table> tail
//   recv <row|host> <pkts> <verdict: 4 B each> <peer_rows: 4 B each> tail
//        -> status (4 B LE each; recv: rotated) | kp | slots | peer_keys | keys | key_peer
// "row" calls the row functions in the order of the host form, "host" the host form itself.
// The output starts as 0xEE.  stdout: one line per call, then "keypairs_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_keypairs.h"

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

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, how;
    if (!(in >> op >> how) || (how != "row" && how != "host")) return 2;
    std::vector<std::vector<uint8_t>> f;
    for (std::string t; in >> t;) f.push_back(unhex(t));
    const size_t head = op == "resp" ? 4 : op == "init" ? 7 : op == "recv" ? 3 : 0;
    if (head == 0 || f.size() != head + 5) return 2;
    const std::vector<uint8_t>* const tf = &f[head];
    if (tf[0].size() % sizeof(wgcs_keypairs) || tf[1].size() % 8 || tf[2].size() % 8 ||
        tf[3].size() % sizeof(wgcs_aead_key) || tf[4].size() != tf[3].size() / sizeof(wgcs_aead_key) * 4)
      return 2;
    const Exact kp_b(tf[0]), slots_b(tf[1]), pk_b(tf[2]), keys_b(tf[3]), key_peer_b(tf[4]);
    auto* const kp = (wgcs_keypairs*)kp_b.p;
    auto* const slots = (wgcs_session_slot*)slots_b.p;
    auto* const pk = (wgcs_session_slot*)pk_b.p;
    auto* const keys = (wgcs_aead_key*)keys_b.p;
    auto* const key_peer = (uint32_t*)key_peer_b.p;
    const uint32_t n_peers = (uint32_t)(kp_b.n / sizeof(wgcs_keypairs)), n_slots = (uint32_t)(slots_b.n / 8);
    const uint32_t n_pk = (uint32_t)(pk_b.n / 8), n_keys = (uint32_t)(keys_b.n / sizeof(wgcs_aead_key));
    std::unique_ptr<Exact> out;
    if (op == "resp") {
      if (f[0].size() % sizeof(wgcs_hs_resp) || f[1].size() != f[0].size() / sizeof(wgcs_hs_resp) * 4 ||
          f[2].size() != 8 || f[3].size() != n_peers * sizeof(wgcs_peer_key))
        return 2;
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_hs_resp));
      int64_t now = 0;
      memcpy(&now, f[2].data(), 8);  // the tests run on little-endian hosts, as the library's layouts assume
      const Exact resp(f[0]), gate(f[1]), table(f[3]);
      out.reset(new Exact(filled(4 * (size_t)n)));
      auto* const st = (int32_t*)out->p;
      const auto* const r = (const wgcs_hs_resp*)resp.p;
      const auto* const g = (const int32_t*)gate.p;
      const auto* const t = (const wgcs_peer_key*)table.p;
      if (how == "host") {
        if (wgcs_keypairs_begin_responder_host(r, g, n, now, t, n_peers, kp, slots, n_slots, pk, n_pk, keys, key_peer,
                                               n_keys, st) != 0)
          return 3;
      } else {
        for (uint32_t j = 0; j < n; ++j) {
          uint32_t x[4];
          st[j] = !keypairs_responder_fields(r, g, j, x)
                      ? WGCS_HS_NONE
                      : keypairs_begin(x[0], x[1], x[2], x[3], false, now, t, n_peers, kp, slots, n_slots, pk, n_pk,
                                       keys, key_peer, n_keys);
        }
      }
    } else if (op == "init") {
      if (f[1].size() % sizeof(wgcs_aead_pkt) || f[2].size() != f[1].size() / sizeof(wgcs_aead_pkt) * 4 ||
          f[3].size() != 8 || f[4].size() % 8 || f[5].size() % sizeof(wgcs_hs_state) ||
          f[6].size() != n_peers * sizeof(wgcs_peer_key))
        return 2;
      const uint32_t n = (uint32_t)(f[1].size() / sizeof(wgcs_aead_pkt));
      int64_t now = 0;
      memcpy(&now, f[3].data(), 8);
      const Exact arena(f[0]), pkts(f[1]), gate(f[2]), hs(f[4]), states(f[5]), table(f[6]);
      out.reset(new Exact(filled(4 * (size_t)n)));
      auto* const st = (int32_t*)out->p;
      const auto* const p = (const wgcs_aead_pkt*)pkts.p;
      const auto* const g = (const int32_t*)gate.p;
      const auto* const h = (const wgcs_session_slot*)hs.p;
      const auto* const s = (const wgcs_hs_state*)states.p;
      const auto* const t = (const wgcs_peer_key*)table.p;
      const uint32_t n_hs = (uint32_t)(hs.n / 8), n_states = (uint32_t)(states.n / sizeof(wgcs_hs_state));
      if (how == "host") {
        if (wgcs_keypairs_begin_initiator_host(arena.p, p, g, n, now, h, n_hs, s, n_states, t, n_peers, kp, slots,
                                               n_slots, pk, n_pk, keys, key_peer, n_keys, st) != 0)
          return 3;
      } else {
        for (uint32_t q = 0; q < n; ++q) {
          uint32_t x[4];
          const int rc = keypairs_initiator_fields(arena.p, p, g, q, h, n_hs, s, n_states, x);
          st[q] = rc != kKeypairsTaken ? rc
                                       : keypairs_begin(x[0], x[1], x[2], x[3], true, now, t, n_peers, kp, slots,
                                                        n_slots, pk, n_pk, keys, key_peer, n_keys);
        }
      }
    } else {
      if (f[0].size() % sizeof(wgcs_aead_pkt) || f[1].size() != f[0].size() / sizeof(wgcs_aead_pkt) * 4 ||
          f[2].size() % 4)
        return 2;
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_aead_pkt)), n_ids = (uint32_t)(f[2].size() / 4);
      const Exact pkts(f[0]), verdict(f[1]), rows(f[2]);
      out.reset(new Exact(filled(4 * (size_t)n)));
      auto* const rot = (uint32_t*)out->p;
      const auto* const p = (const wgcs_aead_pkt*)pkts.p;
      const auto* const v = (const int32_t*)verdict.p;
      const auto* const pr = (const uint32_t*)rows.p;
      if (how == "host") {
        if (wgcs_keypairs_received_host(p, v, n, key_peer, n_keys, pr, n_ids, kp, n_peers, slots, n_slots, pk, n_pk,
                                        keys, rot) != 0)
          return 3;
      } else {
        for (uint32_t i = 0; i < n; ++i)
          rot[i] = keypairs_received_claim(i, p, v, key_peer, n_keys, pr, n_ids, kp, n_peers);
        for (uint32_t i = 0; i < n; ++i)
          if (rot[i])
            rot[i] = keypairs_received_commit(i, p, key_peer, n_keys, pr, n_ids, kp, n_peers, slots, n_slots, pk, n_pk,
                                              keys);
      }
    }
    print_hex(*out);
    for (const Exact* e : {&kp_b, &slots_b, &pk_b, &keys_b, &key_peer_b}) {
      printf(" ");
      print_hex(*e);
    }
    printf("\n");
  }
  printf("keypairs_host: ok\n");
  return 0;
}
