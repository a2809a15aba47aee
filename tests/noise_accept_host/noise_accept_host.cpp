// noise_accept_host.cpp -- drives the responder's stateful tail of wireguard_amd/csrc/wgcs_noise.h
// (noise_accept_claim, noise_accept_verdict, noise_accept_commit, noise_accept_tail) and the host
// functions wgcs_handshake_accept_host / wgcs_peer_rows_build of noise.cpp, the code the lanes of
// hs_accept_claim_kernel, hs_accept_verdict_kernel and hs_accept_commit_kernel run, as plain host
// code (built by tests/test_noise_accept_host.py with -fsanitize=address,undefined together with
// noise.cpp).
//
// Every table is copied into a heap buffer of exactly its size, and every output is a heap
// buffer of exactly its size, so a read or a write past either end is a sanitizer report.
//
// stdin, one case per line, hex fields ("-" = absent: a NULL pointer, no rows):
//   accept <row|host> <init: 128 B each|-> <gate: 4 B each|-> <now: 8 B LE> <table: 72 B each>
//          <peer_rows: 4 B each> <peers: 64 B each> <tickets: 48 B each|->
//        -> verdict (4 B LE each) | peers | resp (80 B each) | count (4 B LE)
//   rows <row|host> <table: 72 B each> <n_ids: 4 B LE>
//        -> rows (4 B LE each)
// "row" calls the row functions in the order of the host form, "host" the host form itself.
// The outputs start as 0xEE.  stdout: one line per case, then "noise_accept_host: ok".
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
    if (op == "accept" && f.size() == 7 && f[0].size() % sizeof(wgcs_hs_init) == 0 &&
        f[1].size() == f[0].size() / sizeof(wgcs_hs_init) * 4 && f[2].size() == 8 &&
        f[3].size() % sizeof(wgcs_peer_key) == 0 && f[4].size() % 4 == 0 && f[5].size() % sizeof(wgcs_hs_peer) == 0 &&
        f[5].size() / sizeof(wgcs_hs_peer) == f[3].size() / sizeof(wgcs_peer_key) &&
        f[6].size() % sizeof(wgcs_hs_ticket) == 0) {
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_hs_init));
      const uint32_t n_peers = (uint32_t)(f[3].size() / sizeof(wgcs_peer_key)), n_ids = (uint32_t)(f[4].size() / 4);
      const uint32_t n_tickets = (uint32_t)(f[6].size() / sizeof(wgcs_hs_ticket));
      int64_t now = 0;
      memcpy(&now, f[2].data(), 8);  // the tests run on little-endian hosts, as the library's layouts assume
      const Exact init(f[0]), gate(f[1]), table(f[3]), rows(f[4]), peers(f[5]), tickets(f[6]),
          resp(filled(sizeof(wgcs_hs_resp) * (size_t)n_tickets)), count(filled(4)), verdict(filled(4 * (size_t)n));
      const auto* const in_rows = (const wgcs_hs_init*)init.p;
      const auto* const g = (const int32_t*)gate.p;
      const auto* const t = (const wgcs_peer_key*)table.p;
      const auto* const pr = (const uint32_t*)rows.p;
      auto* const ps = (wgcs_hs_peer*)peers.p;
      const auto* const tk = (const wgcs_hs_ticket*)tickets.p;
      auto* const r = (wgcs_hs_resp*)resp.p;
      auto* const v = (int32_t*)verdict.p;
      auto* const c = (uint32_t*)count.p;
      if (how == "host") {
        if (wgcs_handshake_accept_host(in_rows, g, n, now, t, pr, n_ids, ps, n_peers, tk, n_tickets, r, c, v) != 0)
          return 3;
      } else {
        for (uint32_t q = 0; q < n; ++q) v[q] = noise_accept_claim(q, in_rows, g, now, t, pr, n_ids, ps, n_peers);
        for (uint32_t q = 0; q < n; ++q) v[q] = noise_accept_verdict(q, v[q], in_rows, n, pr, ps);
        uint32_t winners = 0;
        for (uint32_t q = 0; q < n; ++q)
          if (v[q] == WGCS_HS_ACCEPTED && g[q] == WGCS_HS_CONSUMED)
            v[q] = noise_accept_commit(q, winners++, now, in_rows, pr, ps, tk, n_tickets, r);
        *c = winners < n_tickets ? winners : n_tickets;
        for (uint32_t j = *c; j < n_tickets; ++j) noise_accept_tail(r + j);
      }
      print_hex(verdict);
      printf(" ");
      print_hex(peers);
      printf(" ");
      print_hex(resp);
      printf(" ");
      print_hex(count);
    } else if (op == "rows" && f.size() == 2 && f[0].size() % sizeof(wgcs_peer_key) == 0 && f[1].size() == 4) {
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_peer_key)), n_ids = b2s_load_le32(f[1].data(), 0, 4);
      const Exact table(f[0]), rows(filled(4 * (size_t)n_ids));
      if (wgcs_peer_rows_build((const wgcs_peer_key*)table.p, n, (uint32_t*)rows.p, n_ids) != 0) return 3;
      print_hex(rows);
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("noise_accept_host: ok\n");
  return 0;
}
