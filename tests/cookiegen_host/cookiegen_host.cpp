// cookiegen_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_cookiegen.h and the
// host forms of cookiegen.cpp, the code the lanes of cookiegen_kernels.hip run, as plain host code
// (built by tests/test_cookiegen_host.py with -fsanitize=address,undefined together with cookiegen.cpp).
//
// Every table and every row array is copied into a heap buffer of exactly its size, and every
// output is a heap buffer of exactly its size, so a read or a write past either end -- a probe
// that does not wrap, a message read past the arena's end -- is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = no rows); scalars are little-endian:
//   build host <peer table: 72 B each>                                          -> gen
//   init|resp <row|host> <desc: 96|80 B each> <status: 4 B each> <msgs> <gen>   -> gen
//   consume <row|host> <arena> <pkts: 24 B each> <type: 4 B each> <now: 8 B> <hs_slots> <states>
//           <slots> <key_peer> <peer_rows> <gen> <peers>                        -> verdict | work | gen | peers
//   age <row|host> <now: 8 B> <gen> <peers>                                     -> peers
// "row" calls the row functions in the passes of the host form, "host" the host form itself.
// An output starts as 0xEE.  stdout: one line per call, then "cookiegen_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_cookiegen.h"

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

// claim, then commit over one source
template <class Rows>
static void sent(const Rows& src, const uint8_t* msgs, uint32_t n, wgcs_cookie_gen* g) {
  each(CookieSentClaim<Rows>{src, g}, n);
  each(CookieSentCommit<Rows>{src, msgs, g}, n);
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
    int64_t now = 0;
    if (op == "build") {
      if (f.size() != 1 || f[0].size() % sizeof(wgcs_peer_key)) return 3;
      const uint32_t n = (uint32_t)(f[0].size() / sizeof(wgcs_peer_key));
      Exact table(f[0]), gen(std::vector<uint8_t>((size_t)n * sizeof(wgcs_cookie_gen), 0xEE));
      if (wgcs_cookie_gen_build((const wgcs_peer_key*)table.p, n, (wgcs_cookie_gen*)gen.p) != WGCS_OK) return 4;
      print_hex(gen);
    } else if (op == "init" || op == "resp") {
      const bool resp = op == "resp";
      const size_t row = resp ? sizeof(wgcs_hs_resp) : sizeof(wgcs_hs_start), pitch = resp ? 96 : 160;
      if (f.size() != 4 || f[0].size() % row || f[1].size() != f[0].size() / row * 4 ||
          f[2].size() != f[0].size() / row * pitch || f[3].size() % sizeof(wgcs_cookie_gen))
        return 3;
      const uint32_t n = (uint32_t)(f[0].size() / row), n_peers = (uint32_t)(f[3].size() / sizeof(wgcs_cookie_gen));
      Exact desc(f[0]), status(f[1]), msgs(f[2]), gen(f[3]);
      const int32_t* st = (const int32_t*)status.p;
      wgcs_cookie_gen* g = (wgcs_cookie_gen*)gen.p;
      if (host) {
        const int rc = resp ? wgcs_cookie_responded_host((const wgcs_hs_resp*)desc.p, st, msgs.p, n, g, n_peers)
                            : wgcs_cookie_initiated_host((const wgcs_hs_start*)desc.p, st, msgs.p, n, g, n_peers);
        if (rc != WGCS_OK) return 4;
      } else {
        if (resp) sent(RespondedRows{(const wgcs_hs_resp*)desc.p, st, n_peers}, msgs.p, n, g);
        else sent(InitiatedRows{(const wgcs_hs_start*)desc.p, st, n_peers}, msgs.p, n, g);
      }
      print_hex(gen);
    } else if (op == "consume") {
      if (f.size() != 11 || f[1].size() % sizeof(wgcs_aead_pkt) || f[2].size() != f[1].size() / sizeof(wgcs_aead_pkt) * 4 ||
          !scalar(f[3], &now) || f[4].size() % sizeof(wgcs_session_slot) || f[5].size() % sizeof(wgcs_hs_state) ||
          f[6].size() % sizeof(wgcs_session_slot) || f[7].size() % 4 || f[8].size() % 4 ||
          f[9].size() % sizeof(wgcs_cookie_gen) || f[10].size() != f[9].size())
        return 3;
      const uint32_t n = (uint32_t)(f[1].size() / sizeof(wgcs_aead_pkt));
      Exact arena(f[0]), pkts(f[1]), type(f[2]), hs_slots(f[4]), states(f[5]), slots(f[6]), key_peer(f[7]);
      Exact peer_rows(f[8]), gen(f[9]), peers(f[10]);
      Exact verdict(std::vector<uint8_t>((size_t)n * 4, 0xEE)), work(std::vector<uint8_t>((size_t)n * 16, 0xEE));
      const CookieGenTables t = {(const wgcs_session_slot*)hs_slots.p,
                                 (uint32_t)(f[4].size() / sizeof(wgcs_session_slot)),
                                 (const wgcs_hs_state*)states.p,
                                 (uint32_t)(f[5].size() / sizeof(wgcs_hs_state)),
                                 (const wgcs_session_slot*)slots.p,
                                 (uint32_t)(f[6].size() / sizeof(wgcs_session_slot)),
                                 (const uint32_t*)key_peer.p,
                                 (uint32_t)(f[7].size() / 4),
                                 (const uint32_t*)peer_rows.p,
                                 (uint32_t)(f[8].size() / 4),
                                 (uint32_t)(f[9].size() / sizeof(wgcs_cookie_gen))};
      const wgcs_aead_pkt* pk = (const wgcs_aead_pkt*)pkts.p;
      const int32_t* ty = (const int32_t*)type.p;
      wgcs_cookie_gen* g = (wgcs_cookie_gen*)gen.p;
      wgcs_hs_peer* ps = (wgcs_hs_peer*)peers.p;
      int32_t* v = (int32_t*)verdict.p;
      if (host) {
        if (wgcs_cookie_consume_host(arena.p, pk, ty, n, now, t.hs_slots, t.n_hs_slots, t.states, t.n_states, t.slots,
                                     t.n_slots, t.key_peer, t.n_keys, t.peer_rows, t.n_ids, g, ps, t.n_peers, work.p,
                                     v) != WGCS_OK)
          return 4;
      } else {
        each(CookieOpen{arena.p, pk, ty, t, g, (uint32_t*)work.p, v}, n);
        each(CookieCommit{arena.p, pk, v, t, now, g, ps, (uint32_t*)work.p}, n);
      }
      print_hex(verdict);
      printf(" ");
      print_hex(work);
      printf(" ");
      print_hex(gen);
      printf(" ");
      print_hex(peers);
    } else if (op == "age") {
      if (f.size() != 3 || !scalar(f[0], &now) || f[1].size() % sizeof(wgcs_cookie_gen) || f[2].size() != f[1].size())
        return 3;
      const uint32_t n_peers = (uint32_t)(f[1].size() / sizeof(wgcs_cookie_gen));
      Exact gen(f[1]), peers(f[2]);
      if (host) {
        if (wgcs_cookie_age_host(now, (const wgcs_cookie_gen*)gen.p, (wgcs_hs_peer*)peers.p, n_peers) != WGCS_OK) return 4;
      } else {
        each(CookieAge{now, (const wgcs_cookie_gen*)gen.p, (wgcs_hs_peer*)peers.p}, n_peers);
      }
      print_hex(peers);
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("cookiegen_host: ok\n");
  return 0;
}
