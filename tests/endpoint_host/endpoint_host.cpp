// endpoint_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_endpoint.h and the host
// forms of endpoint.cpp, the code the lanes of endpoint_kernels.hip run, as plain host code (built
// by tests/test_endpoint_host.py with -fsanitize=address,undefined together with endpoint.cpp).
//
// Every table and every row array is copied into a heap buffer of exactly its size, and every
// output is a heap buffer of exactly its size, so a read or a write past either end -- a control
// message read past its slot, a source row past d_ep, a job's lengths past its segments -- is a
// sanitizer report.
//
// stdin, one call per line, hex fields ("-" = no rows); scalars are little-endian 4-byte words:
//   gso host <control>                                                     -> rc | gso
//   recv <row|host> <addr> <from> <size> <oob> <oob_stride> <nn> <n_msgs>   -> ep | addr_out
//   received <row|host> <groups> <calls_per_batch> <ep> <peer_rows> <table> <claim> <timers>
//   accepted <row|host> <resp> <ep> <table> <claim> <timers>
//   finished <row|host> <arena> <pkts> <gate> <hs_slots> <states> <ep> <table> <claim> <timers>
//                                                                          -> table | claim | timers
//   jobs <row|host> <peer> <count> <status> <job_key> <max_segs> <lens> <nbufs> <peer_rows> <table> <timers>
//                                                                          -> dst | v6 | status | tx | nbufs | table | timers
//   init|resp <row|host> <desc> <status> <table> <timers>                  -> dst | v6 | status | table | timers
// "row" calls the row functions in the passes of the host form, "host" the host form itself.
// An output starts as 0xEE.  stdout: one line per call, then "endpoint_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_endpoint.h"

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

static void print_hex(const Exact& e, bool more = true) {
  if (e.n == 0) printf("-");
  for (size_t i = 0; i < e.n; ++i) printf("%02x", e.p[i]);
  if (more) printf(" ");
}

static bool word(const std::vector<uint8_t>& f, uint32_t* out) {
  if (f.size() != 4) return false;
  memcpy(out, f.data(), 4);
  return true;
}

// a body of the header for every entry in order, as the host forms run it
template <class F>
static void each(const F& f, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) f(i);
}

template <class Rows>
static void set_rows(const Rows& src, uint32_t n, const wgcs_endpoint* ep, uint32_t n_rows, wgcs_endpoint* table,
                     uint32_t* claim, wgcs_timers* timers) {
  each(EndpointSetClaim<Rows>{src, ep, n_rows, claim}, n);
  each(EndpointSetCommit<Rows>{src, ep, n_rows, table, claim, timers}, n);
}

template <class Rows>
static void dst_rows(const Rows& src, uint32_t n, wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst,
                     int32_t* dst_v6, int32_t* dst_status) {
  each(EndpointDstRead<Rows>{src, table, timers, dst, dst_v6, dst_status}, n);
  each(EndpointDstClear<Rows>{src, table, timers}, n);
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
    if (op == "gso") {
      if (f.size() != 1) return 3;
      Exact control(f[0]);
      int gso = -1;
      const int rc = wgcs::cmsg_gso_size(control.p, control.n, &gso);
      printf("%d %d", rc, gso);
    } else if (op == "recv") {
      uint32_t stride, n_msgs;
      if (f.size() != 7 || !word(f[4], &stride) || !word(f[6], &n_msgs) || n_msgs == 0 || f[2].size() % (4 * n_msgs)) return 3;
      const uint32_t n = (uint32_t)(f[2].size() / 4);
      if (f[0].size() != n * sizeof(wgcs_src_addr) || (f[1].size() && f[1].size() != n * 4) || f[3].size() != (size_t)n * stride ||
          f[5].size() != n * 4)
        return 3;
      Exact addr(f[0]), from(f[1]), size(f[2]), oob(f[3]), nn(f[5]);
      Exact ep((size_t)n * sizeof(wgcs_endpoint)), out((size_t)n * sizeof(wgcs_src_addr));
      if (host) {
        if (wgcs_endpoint_recv_host((const wgcs_src_addr*)addr.p, (const int32_t*)from.p, (const int32_t*)size.p, oob.p,
                                    stride, (const int32_t*)nn.p, n_msgs, n / n_msgs, (wgcs_endpoint*)ep.p,
                                    (wgcs_src_addr*)out.p) != WGCS_OK)
          return 4;
      } else {
        each(EndpointRecv{n_msgs, (const wgcs_src_addr*)addr.p, (const int32_t*)from.p, (const int32_t*)size.p, oob.p,
                          stride, (const int32_t*)nn.p, (wgcs_endpoint*)ep.p, (wgcs_src_addr*)out.p},
             n);
      }
      print_hex(ep);
      print_hex(out, false);
    } else if (op == "received" || op == "accepted" || op == "finished") {
      const size_t k = op == "received" ? 4 : op == "accepted" ? 2 : 6;  // where table | claim | timers start
      if (f.size() != k + 3 || f[k].size() % sizeof(wgcs_endpoint) || f[k + 1].size() != f[k].size() / 16 ||
          f[k + 2].size() != f[k].size())
        return 3;
      const uint32_t n_peers = (uint32_t)(f[k].size() / sizeof(wgcs_endpoint));
      Exact table(f[k]), claim(f[k + 1]), timers(f[k + 2]), ep(f[op == "received" ? 2 : k - 1]);
      wgcs_endpoint* const t = (wgcs_endpoint*)table.p;
      uint32_t* const c = (uint32_t*)claim.p;
      wgcs_timers* const tm = (wgcs_timers*)timers.p;
      const wgcs_endpoint* const e = (const wgcs_endpoint*)ep.p;
      const uint32_t n_rows = (uint32_t)(ep.n / sizeof(wgcs_endpoint));
      if (op == "received") {
        uint32_t cpb;
        if (!word(f[1], &cpb) || cpb == 0 || f[0].size() % (sizeof(wgcs_write_group) * cpb) || f[3].size() % 4) return 3;
        Exact groups(f[0]), peer_rows(f[3]);
        const uint32_t n = (uint32_t)(groups.n / sizeof(wgcs_write_group)), n_ids = (uint32_t)(peer_rows.n / 4);
        if (host) {
          if (wgcs_endpoint_set_received_host((const wgcs_write_group*)groups.p, n / cpb, cpb, e, n_rows,
                                              (const uint32_t*)peer_rows.p, n_ids, t, c, tm, n_peers) != WGCS_OK)
            return 4;
        } else {
          set_rows(GroupRows{(const wgcs_write_group*)groups.p, (const uint32_t*)peer_rows.p, n_ids, n_peers}, n, e,
                   n_rows, t, c, tm);
        }
      } else if (op == "accepted") {
        if (f[0].size() % sizeof(wgcs_hs_resp)) return 3;
        Exact resp(f[0]);
        const uint32_t n = (uint32_t)(resp.n / sizeof(wgcs_hs_resp));
        if (host) {
          if (wgcs_endpoint_set_accepted_host((const wgcs_hs_resp*)resp.p, n, e, n_rows, t, c, tm, n_peers) != WGCS_OK) return 4;
        } else {
          set_rows(AcceptedRows{(const wgcs_hs_resp*)resp.p, n_peers}, n, e, n_rows, t, c, tm);
        }
      } else {
        if (f[1].size() % sizeof(wgcs_aead_pkt) || f[2].size() != f[1].size() / sizeof(wgcs_aead_pkt) * 4 ||
            f[3].size() % sizeof(wgcs_session_slot) || f[4].size() % sizeof(wgcs_hs_state))
          return 3;
        Exact arena(f[0]), pkts(f[1]), gate(f[2]), hs_slots(f[3]), states(f[4]);
        const uint32_t n = (uint32_t)(pkts.n / sizeof(wgcs_aead_pkt));
        const uint32_t n_hs = (uint32_t)(hs_slots.n / sizeof(wgcs_session_slot)), n_st = (uint32_t)(states.n / sizeof(wgcs_hs_state));
        if (n_rows != n) return 3;
        if (host) {
          if (wgcs_endpoint_set_finished_host(arena.p, (const wgcs_aead_pkt*)pkts.p, (const int32_t*)gate.p, n,
                                              (const wgcs_session_slot*)hs_slots.p, n_hs, (const wgcs_hs_state*)states.p,
                                              n_st, e, t, c, tm, n_peers) != WGCS_OK)
            return 4;
        } else {
          set_rows(FinishedRows{arena.p, (const wgcs_aead_pkt*)pkts.p, (const int32_t*)gate.p,
                                (const wgcs_session_slot*)hs_slots.p, n_hs, (const wgcs_hs_state*)states.p, n_st,
                                n_peers},
                   n, e, n, t, c, tm);
        }
      }
      print_hex(table);
      print_hex(claim);
      print_hex(timers, false);
    } else if (op == "jobs") {
      uint32_t max_segs;
      if (f.size() != 10 || !word(f[4], &max_segs) || max_segs == 0 || f[1].size() % 4 || f[7].size() % 4 ||
          f[8].size() % sizeof(wgcs_endpoint) || f[9].size() != f[8].size())
        return 3;
      const uint32_t n = (uint32_t)(f[1].size() / 4), n_ids = (uint32_t)(f[7].size() / 4);
      const uint32_t n_peers = (uint32_t)(f[8].size() / sizeof(wgcs_endpoint));
      if (f[0].size() != (size_t)n * max_segs * 4 || f[2].size() != n * 4 || f[3].size() != n * 4 ||
          f[5].size() != (size_t)n * max_segs * 4 || f[6].size() != n * 4)
        return 3;
      Exact peer(f[0]), count(f[1]), status(f[2]), key(f[3]), lens(f[5]), nbufs(f[6]), peer_rows(f[7]), table(f[8]), timers(f[9]);
      Exact dst((size_t)n * sizeof(wgcs_endpoint)), v6((size_t)n * 4), ds((size_t)n * 4), tx((size_t)n * 8);
      wgcs_endpoint* const t = (wgcs_endpoint*)table.p;
      wgcs_timers* const tm = (wgcs_timers*)timers.p;
      if (host) {
        if (wgcs_endpoint_dst_jobs_host((const uint32_t*)peer.p, (const int32_t*)count.p, (const int32_t*)status.p,
                                        (const uint32_t*)key.p, n, max_segs, (const int32_t*)lens.p, (int32_t*)nbufs.p,
                                        (const uint32_t*)peer_rows.p, n_ids, t, tm, n_peers, (wgcs_endpoint*)dst.p,
                                        (int32_t*)v6.p, (int32_t*)ds.p, (uint64_t*)tx.p) != WGCS_OK)
          return 4;
      } else {
        const KeptJobRows fj = {{(const uint32_t*)peer.p, (const int32_t*)count.p, (const int32_t*)status.p, max_segs,
                                 (const uint32_t*)peer_rows.p, n_ids, n_peers},
                                (const uint32_t*)key.p};
        each(EndpointDstJobs{{fj, t, tm, (wgcs_endpoint*)dst.p, (int32_t*)v6.p, (int32_t*)ds.p}, (const int32_t*)lens.p,
                             (int32_t*)nbufs.p, (uint64_t*)tx.p},
             n);
        each(EndpointDstClear<KeptJobRows>{fj, t, tm}, n);
      }
      print_hex(dst);
      print_hex(v6);
      print_hex(ds);
      print_hex(tx);
      print_hex(nbufs);
      print_hex(table);
      print_hex(timers, false);
    } else if (op == "init" || op == "resp") {
      const bool resp = op == "resp";
      const size_t rowsz = resp ? sizeof(wgcs_hs_resp) : sizeof(wgcs_hs_start);
      if (f.size() != 4 || f[0].size() % rowsz || f[1].size() != f[0].size() / rowsz * 4 ||
          f[2].size() % sizeof(wgcs_endpoint) || f[3].size() != f[2].size())
        return 3;
      const uint32_t n = (uint32_t)(f[0].size() / rowsz), n_peers = (uint32_t)(f[2].size() / sizeof(wgcs_endpoint));
      Exact desc(f[0]), status(f[1]), table(f[2]), timers(f[3]);
      Exact dst((size_t)n * sizeof(wgcs_endpoint)), v6((size_t)n * 4), ds((size_t)n * 4);
      wgcs_endpoint* const t = (wgcs_endpoint*)table.p;
      wgcs_timers* const tm = (wgcs_timers*)timers.p;
      const int32_t* const st = (const int32_t*)status.p;
      if (host) {
        const int rc = resp ? wgcs_endpoint_dst_responded_host((const wgcs_hs_resp*)desc.p, st, n, t, tm, n_peers,
                                                               (wgcs_endpoint*)dst.p, (int32_t*)v6.p, (int32_t*)ds.p)
                            : wgcs_endpoint_dst_initiated_host((const wgcs_hs_start*)desc.p, st, n, t, tm, n_peers,
                                                               (wgcs_endpoint*)dst.p, (int32_t*)v6.p, (int32_t*)ds.p);
        if (rc != WGCS_OK) return 4;
      } else {
        wgcs_endpoint* const d = (wgcs_endpoint*)dst.p;
        int32_t *const d6 = (int32_t*)v6.p, *const dstat = (int32_t*)ds.p;
        if (resp) dst_rows(RespondedRows{(const wgcs_hs_resp*)desc.p, st, n_peers}, n, t, tm, d, d6, dstat);
        else dst_rows(InitiatedRows{(const wgcs_hs_start*)desc.p, st, n_peers}, n, t, tm, d, d6, dstat);
      }
      print_hex(dst);
      print_hex(v6);
      print_hex(ds);
      print_hex(table);
      print_hex(timers, false);
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("endpoint_host: ok\n");
  return 0;
}
