// staged_host.cpp -- drives the host forms of staged.cpp, which run the row functions of
// wireguard_amd/csrc/wgcs_staged.h, the code the lanes of staged_kernels.hip run, as plain host
// code (built by tests/test_staged_host.py with -fsanitize=address,undefined together with staged.cpp).
//
// Every table, the arena, the ring, the job table and the scratch are heap buffers of exactly
// their size -- the last slot ends where its buffer ends -- so a ring position that is not masked,
// a slot index past the table or a copy of one byte too many is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = no rows); scalars are little-endian:
//   stage <stride: 8 B> <max_segs: 4 B> <cap: 4 B> <arena> <sizes> <peer> <count> <status_in> <status_out>
//         <job_key> <peer_rows> <len> <head> <lost> <slot_size> <ring>   -> where | len | head | lost | slot_size | ring
//   release <now: 8 B> <limit: 8 B> <stride: 8 B> <cap: 4 B> <n_out_max: 4 B> <table: 72 B each> <kp: 80 B each>
//         <send_nonce> <rekey> <len> <head> <slot_size> <ring>
//                        -> status | n_out | out | out_peer | out_count | out_sizes | out_status | rekey | len | head
//   flush <all: 4 B, 1 = no actions> <actions> <len> <head> <lost>       -> len | head | lost
// An output starts as 0xEE.  stdout: one line per call, then "staged_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_staged.h"

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
  Exact(size_t bytes) : Exact(std::vector<uint8_t>(bytes, 0xEE)) {}
};

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static void print_hex(const Exact& e, const char* sep = " ") {
  if (e.n == 0) printf("-");
  for (size_t i = 0; i < e.n; ++i) printf("%02x", e.p[i]);
  printf("%s", sep);
}

template <typename T>
static bool scalar(const std::vector<uint8_t>& f, T* out) {
  if (f.size() != sizeof(T)) return false;
  memcpy(out, f.data(), sizeof(T));
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) return 2;
    std::vector<std::vector<uint8_t>> f;
    for (std::string t; in >> t;) f.push_back(unhex(t));
    if (op == "stage") {
      uint64_t stride;
      uint32_t max_segs, cap;
      if (f.size() != 16 || !scalar(f[0], &stride) || !scalar(f[1], &max_segs) || !scalar(f[2], &cap)) return 3;
      const uint32_t n_jobs = (uint32_t)(f[6].size() / 4), n_peers = (uint32_t)(f[11].size() / 4);
      if (f[3].size() != (size_t)n_jobs * max_segs * stride || f[4].size() != (size_t)n_jobs * max_segs * 4 ||
          f[15].size() != (size_t)n_peers * cap * stride || f[14].size() != (size_t)n_peers * cap * 4)
        return 3;
      Exact arena(f[3]), sizes(f[4]), peer(f[5]), count(f[6]), status_in(f[7]), status_out(f[8]), job_key(f[9]);
      Exact peer_rows(f[10]), len(f[11]), head(f[12]), lost(f[13]), slot_size(f[14]), ring(f[15]);
      Exact where((size_t)n_jobs * max_segs * 4), work(staged_stage_host_work_bytes(n_jobs));
      if (wgcs_staged_stage_host(arena.p, stride, (const int32_t*)sizes.p, (const uint32_t*)peer.p,
                                 (const int32_t*)count.p, (const int32_t*)status_in.p, (const int32_t*)status_out.p,
                                 (const uint32_t*)job_key.p, n_jobs, max_segs, (const uint32_t*)peer_rows.p,
                                 (uint32_t)(f[10].size() / 4), (uint32_t*)len.p, (uint32_t*)head.p, (uint32_t*)lost.p,
                                 (int32_t*)slot_size.p, ring.p, n_peers, cap, (uint32_t*)where.p, work.p,
                                 work.n) != WGCS_OK)
        return 4;
      print_hex(where), print_hex(len), print_hex(head), print_hex(lost), print_hex(slot_size), print_hex(ring, "");
    } else if (op == "release") {
      int64_t now;
      uint64_t limit, stride;
      uint32_t cap, n_out_max;
      if (f.size() != 13 || !scalar(f[0], &now) || !scalar(f[1], &limit) || !scalar(f[2], &stride) ||
          !scalar(f[3], &cap) || !scalar(f[4], &n_out_max) || f[5].size() % sizeof(wgcs_peer_key))
        return 3;
      const uint32_t n_peers = (uint32_t)(f[5].size() / sizeof(wgcs_peer_key));
      if (f[6].size() != (size_t)n_peers * sizeof(wgcs_keypairs) || f[8].size() != (size_t)n_peers * sizeof(wgcs_rekey) ||
          f[9].size() != (size_t)n_peers * 4 || f[12].size() != (size_t)n_peers * cap * stride)
        return 3;
      Exact table(f[5]), kp(f[6]), nonce(f[7]), rekey(f[8]), len(f[9]), head(f[10]), slot_size(f[11]), ring(f[12]);
      Exact status((size_t)n_peers * 4), n_out(4), out((size_t)n_out_max * stride), out_peer((size_t)n_out_max * 4);
      Exact out_count((size_t)n_out_max * 4), out_sizes((size_t)n_out_max * 4), out_status((size_t)n_out_max * 4);
      if (wgcs_staged_release_host(now, (const wgcs_peer_key*)table.p, (const wgcs_keypairs*)kp.p,
                                   (const uint64_t*)nonce.p, (uint32_t)(f[7].size() / 8), limit, (wgcs_rekey*)rekey.p,
                                   (uint32_t*)len.p, (uint32_t*)head.p, (const int32_t*)slot_size.p, ring.p, n_peers,
                                   cap, stride, n_out_max, out.p, (uint32_t*)out_peer.p, (int32_t*)out_count.p,
                                   (int32_t*)out_sizes.p, (int32_t*)out_status.p, (uint32_t*)n_out.p,
                                   (int32_t*)status.p) != WGCS_OK)
        return 4;
      print_hex(status), print_hex(n_out), print_hex(out), print_hex(out_peer), print_hex(out_count);
      print_hex(out_sizes), print_hex(out_status), print_hex(rekey), print_hex(len), print_hex(head, "");
    } else if (op == "flush") {
      uint32_t all;
      if (f.size() != 5 || !scalar(f[0], &all) || f[3].size() != f[2].size() || f[4].size() != f[2].size()) return 3;
      Exact actions(f[1]), len(f[2]), head(f[3]), lost(f[4]);
      if (wgcs_staged_flush_host(all ? nullptr : (const uint32_t*)actions.p, (uint32_t*)len.p, (uint32_t*)head.p,
                                 (uint32_t*)lost.p, (uint32_t)(f[2].size() / 4)) != WGCS_OK)
        return 4;
      print_hex(len), print_hex(head), print_hex(lost, "");
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("staged_host: ok\n");
  return 0;
}
