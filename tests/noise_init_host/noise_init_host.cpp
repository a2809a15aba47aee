// noise_init_host.cpp -- drives the initiator's half of wireguard_amd/csrc/wgcs_noise.h
// (noise_initiate_row, noise_finish_row with noise_finish_commit) and the host forms
// wgcs_handshake_initiate_host / wgcs_handshake_finish_host of noise.cpp, the code the lanes
// of hs_initiate_kernel, hs_finish_kernel and hs_finish_commit_kernel run, as plain host code
// (built by tests/test_noise_init_host.py with -fsanitize=address,undefined together with
// noise.cpp).
//
// Every table is copied into a heap buffer of exactly its size, and every output is a heap
// buffer of exactly its size, so a read or a write past either end is a sanitizer report.
//
// stdin, one case per line, hex fields ("-" = absent: a NULL pointer, no rows):
//   initiate <row|host> <start: 96 B each> <static public:32B> <table: 72 B each> <n_keys:4B LE>
//            <states: 128 B each>
//        -> status (4 B LE each) | msgs (160 B each) | states
//   finish <row|host> <arena> <pkts: 24 B each> <types: 4 B each> <gate: 4 B each|-> <responder:96B>
//          <slots: 8 B each|-> <states: 128 B each> <psk: 32 B each|-> <n_peers:4B LE> <keys: 48 B each>
//        -> verdict (4 B LE each) | states | keys | work (64 B each)
// "row" calls the row functions in the order of the host form, "host" the host form itself.
// The outputs start as 0xEE.  stdout: one line per case, then "noise_init_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_noise.h"

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
  for (size_t i = 0; i < e.n; ++i) printf("%02x", e.p[i]);
}

static std::vector<uint8_t> filled(size_t n) { return std::vector<uint8_t>(n, 0xEE); }

static uint32_t le32(const std::vector<uint8_t>& v) { return b2s_load_le32(v.data(), 0, 4); }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, how;
    if (!(in >> op >> how) || (how != "row" && how != "host")) return 2;
    std::vector<std::vector<uint8_t>> f;
    for (std::string t; in >> t;) f.push_back(unhex(t));
    if (op == "initiate" && f.size() == 5 && f[0].size() % sizeof(wgcs_hs_start) == 0 && f[1].size() == 32 &&
        f[2].size() % sizeof(wgcs_peer_key) == 0 && f[3].size() == 4 && f[4].size() % sizeof(wgcs_hs_state) == 0) {
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_hs_start));
      const uint32_t n_peers = (uint32_t)(f[2].size() / sizeof(wgcs_peer_key));
      const uint32_t n_states = (uint32_t)(f[4].size() / sizeof(wgcs_hs_state)), n_keys = le32(f[3]);
      const Exact start(f[0]), pub(f[1]), table(f[2]), states(f[4]), msgs(filled(kNoiseInitiationPitch * (size_t)n)),
          status(filled(4 * (size_t)n));
      const auto* const d = (const wgcs_hs_start*)start.p;
      const auto* const t = (const wgcs_peer_key*)table.p;
      auto* const st = (wgcs_hs_state*)states.p;
      if (how == "host") {
        if (wgcs_handshake_initiate_host(d, n, pub.p, t, n_peers, n_keys, st, n_states, msgs.p, (int32_t*)status.p) != 0)
          return 3;
      } else {
        for (uint32_t q = 0; q < n; ++q)
          ((int32_t*)status.p)[q] = noise_initiate_row(d + q, pub.p, t, n_peers, n_keys, st, n_states,
                                                       msgs.p + kNoiseInitiationPitch * (size_t)q);
      }
      print_hex(status);
      printf(" ");
      print_hex(msgs);
      printf(" ");
      print_hex(states);
    } else if (op == "finish" && f.size() == 10 && f[1].size() % sizeof(wgcs_aead_pkt) == 0 &&
               f[2].size() == f[1].size() / sizeof(wgcs_aead_pkt) * 4 && (f[3].empty() || f[3].size() == f[2].size()) &&
               f[4].size() == sizeof(wgcs_noise_responder) && f[5].size() % sizeof(wgcs_session_slot) == 0 &&
               f[6].size() % sizeof(wgcs_hs_state) == 0 && f[7].size() % 32 == 0 && f[8].size() == 4 &&
               f[9].size() % sizeof(wgcs_aead_key) == 0) {
      const uint32_t n = (uint32_t)(f[1].size() / sizeof(wgcs_aead_pkt));
      const uint32_t n_slots = (uint32_t)(f[5].size() / sizeof(wgcs_session_slot));
      const uint32_t n_states = (uint32_t)(f[6].size() / sizeof(wgcs_hs_state)), n_peers = le32(f[8]);
      const uint32_t n_keys = (uint32_t)(f[9].size() / sizeof(wgcs_aead_key));
      const Exact arena(f[0]), pkts(f[1]), types(f[2]), gate(f[3]), self(f[4]), slots(f[5]), states(f[6]), psk(f[7]),
          keys(f[9]), work(filled(4 * kHsWorkWords * (size_t)n)), verdict(filled(4 * (size_t)n));
      const auto* const pk = (const wgcs_aead_pkt*)pkts.p;
      const auto* const ty = (const int32_t*)types.p;
      const auto* const g = (const int32_t*)gate.p;
      const auto* const me = (const wgcs_noise_responder*)self.p;
      const auto* const sl = (const wgcs_session_slot*)slots.p;
      auto* const st = (wgcs_hs_state*)states.p;
      auto* const ks = (wgcs_aead_key*)keys.p;
      auto* const v = (int32_t*)verdict.p;
      if (how == "host") {
        if (wgcs_handshake_finish_host(arena.p, pk, ty, g, n, me, sl, n_slots, st, n_states, psk.p, n_peers, ks, n_keys,
                                       work.p, v) != 0)
          return 3;
      } else {
        for (uint32_t q = 0; q < n; ++q)
          v[q] = noise_finish_row(q, arena.p, pk, ty, g, me, sl, n_slots, st, n_states, psk.p, n_peers, n_keys, work.p);
        for (uint32_t q = 0; q < n; ++q) v[q] = noise_finish_commit(q, v[q], arena.p, pk, sl, n_slots, st, ks, work.p);
      }
      print_hex(verdict);
      printf(" ");
      print_hex(states);
      printf(" ");
      print_hex(keys);
      printf(" ");
      print_hex(work);
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("noise_init_host: ok\n");
  return 0;
}
