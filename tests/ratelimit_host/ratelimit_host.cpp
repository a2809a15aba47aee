// ratelimit_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_ratelimit.h and the
// host forms of ratelimit.cpp, the code the lanes of ratelimit_kernels.hip run, as plain host code
// (built by tests/test_ratelimit_host.py with -fsanitize=address,undefined together with ratelimit.cpp).
//
// Every table and every row array is copied into a heap buffer of exactly its size, and every
// output is a heap buffer of exactly its size, so a read or a write past either end -- a probe
// that does not wrap, a look past the last position -- is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = no rows); scalars are little-endian:
//   batch <row|host> <gate: 4 B each> <src: 20 B each> <table: 40 B each> <now: 8 B>  -> verdict | stats | table
//   clean <row|host> <table> <now>                                                    -> live | new table
//   allow host <src: 20 B> <table> <now>                                              -> rc (4 B) | table
//   home  host <src: 20 B> <n_slots: 4 B>                                             -> slot (4 B)
// "row" calls the row functions in the passes of the host form, "host" the host form itself.
// An output starts as 0xEE.  stdout: one line per call, then "ratelimit_host: ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_ratelimit.h"

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

template <typename T>
static Exact of_scalar(T v) {
  std::vector<uint8_t> b(sizeof(T));
  memcpy(b.data(), &v, sizeof(T));
  return Exact(b);
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
    if (op == "batch") {
      if (f.size() != 4 || f[0].size() % 4 || f[1].size() != f[0].size() * 5 || f[2].size() % sizeof(wgcs_rl_entry) ||
          !scalar(f[3], &now))
        return 3;
      const uint32_t n = (uint32_t)(f[0].size() / 4), n_slots = (uint32_t)(f[2].size() / sizeof(wgcs_rl_entry));
      Exact gate(f[0]), src(f[1]), table(f[2]);
      Exact verdict(std::vector<uint8_t>(f[0].size(), 0xEE)), stats(std::vector<uint8_t>(16, 0xEE));
      const int32_t* g = (const int32_t*)gate.p;
      const wgcs_src_addr* s = (const wgcs_src_addr*)src.p;
      wgcs_rl_entry* t = (wgcs_rl_entry*)table.p;
      int32_t* v = (int32_t*)verdict.p;
      if (host) {
        if (wgcs_ratelimit_batch_host(g, s, n, t, n_slots, now, v, (uint32_t*)stats.p) != WGCS_OK) return 4;
      } else {
        uint32_t counts[kRlStats] = {0, 0, 0, 0};
        Exact keys_in(std::vector<uint8_t>(f[0].size(), 0xEE)), keys(std::vector<uint8_t>(f[0].size(), 0xEE));
        Exact slots(std::vector<uint8_t>(f[0].size(), 0xEE));
        uint32_t *ki = (uint32_t*)keys_in.p, *k = (uint32_t*)keys.p, *sl = (uint32_t*)slots.p;
        for (uint32_t q = 0; q < n; ++q) {
          bool full = false;
          ki[q] = rl_find_or_claim(q, g, s, n, t, n_slots, v, &full);
          counts[kRlTableFull] += full;
          sl[q] = q;
        }
        if (n) std::stable_sort(sl, sl + n, [&](uint32_t a, uint32_t b) { return ki[a] < ki[b]; });
        for (uint32_t p = 0; p < n; ++p) k[p] = ki[sl[p]];
        for (uint32_t p = 0; p < n; ++p) rl_position(p, k, sl, n, n_slots, s, t, now, v, counts);
        memcpy(stats.p, counts, sizeof counts);
      }
      print_hex(verdict);
      printf(" ");
      print_hex(stats);
      printf(" ");
      print_hex(table);
    } else if (op == "clean") {
      if (f.size() != 2 || f[0].empty() || f[0].size() % sizeof(wgcs_rl_entry) || !scalar(f[1], &now)) return 3;
      const uint32_t n_slots = (uint32_t)(f[0].size() / sizeof(wgcs_rl_entry));
      Exact old_table(f[0]), new_table(std::vector<uint8_t>(f[0].size(), 0xEE));
      uint32_t live = 0xEEEEEEEEu;
      const wgcs_rl_entry* o = (const wgcs_rl_entry*)old_table.p;
      wgcs_rl_entry* t = (wgcs_rl_entry*)new_table.p;
      if (host) {
        if (wgcs_ratelimit_cleanup_host(o, t, n_slots, now, &live) != WGCS_OK) return 4;
      } else {
        memset(t, 0, new_table.n);
        live = 0;
        for (uint32_t i = 0; i < n_slots; ++i) live += rl_cleanup_row(i, o, t, n_slots, now);
      }
      print_hex(of_scalar(live));
      printf(" ");
      print_hex(new_table);
    } else if (op == "allow") {
      if (f.size() != 3 || f[0].size() != sizeof(wgcs_src_addr) || f[1].size() % sizeof(wgcs_rl_entry) ||
          !scalar(f[2], &now))
        return 3;
      Exact src(f[0]), table(f[1]);
      const int32_t rc = wgcs_ratelimit_allow((wgcs_rl_entry*)table.p, (uint32_t)(f[1].size() / sizeof(wgcs_rl_entry)),
                                              (const wgcs_src_addr*)src.p, now);
      print_hex(of_scalar(rc));
      printf(" ");
      print_hex(table);
    } else if (op == "home") {
      uint32_t n_slots = 0;
      if (f.size() != 2 || f[0].size() != sizeof(wgcs_src_addr) || !scalar(f[1], &n_slots)) return 3;
      Exact src(f[0]);
      print_hex(of_scalar(wgcs_ratelimit_home_slot((const wgcs_src_addr*)src.p, n_slots)));
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("ratelimit_host: ok\n");
  return 0;
}
