// rekey_host.cpp -- drives the row functions of wireguard_amd/csrc/wgcs_rekey.h and the six
// wgcs_rekey_*_host forms of rekey.cpp, the code the lanes of rekey_kernels.hip run, as plain host
// code (built by tests/test_rekey_host.py with -fsanitize=address,undefined together with rekey.cpp).
//
// Every table is copied into a heap buffer of exactly its size, and every output is a heap
// buffer of exactly its size, so a read or a write past either end is a sanitizer report.
//
// stdin, one call per line, hex fields ("-" = absent: a NULL pointer, no rows); scalars are little-endian:
//   recv  <row|host> <pkts: 24 B each> <now: 8 B> <key_peer: 4 B each> <peer_rows: 4 B each> <kp: 80 B each>
//         -> pkts
//   gate  <row|host> <peer: 4 B each> <count: 4 B each> <status_in: 4 B each> <max_segs: 4 B> <now> <peer_rows> <kp>
//         <send_nonce: 8 B each> <limit: 8 B> <rekey: 16 B each>       -> status_out | rekey
//   sent  <row|host> <peer> <count> <status> <job_key: 4 B each> <max_segs> <now> <peer_rows> <kp> <send_nonce>
//         <limit> <rekey>                                              -> rekey
//   rcvd  <row|host> <groups: 24 B each> <calls_per_batch: 4 B> <now> <peer_rows> <kp> <rekey>    -> rekey
//   resp  <row|host> <resp: 80 B each> <gate: 4 B each> <now> <rekey>                             -> rekey
//   start <row|host> <now> <rekey> <hs_peers: 64 B each> <tickets: 96 B each>
//         -> status | reasons | start | start_peer | count | rekey
// "row" calls the row functions in the order of the host form, "host" the host form itself.
// An output starts as 0xEE.  stdout: one line per call, then "rekey_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_rekey.h"

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
    if (op == "recv") {
      if (f.size() != 5 || f[0].size() % sizeof(wgcs_aead_pkt) || !scalar(f[1], &now) || f[2].size() % 4 ||
          f[3].size() % 4 || f[4].size() % sizeof(wgcs_keypairs))
        return 2;
      const Exact *pkts = exact(f[0]), *key_peer = exact(f[2]), *rows = exact(f[3]), *kp = exact(f[4]);
      const uint32_t n = (uint32_t)(pkts->n / sizeof(wgcs_aead_pkt)), n_keys = (uint32_t)(key_peer->n / 4);
      const uint32_t n_ids = (uint32_t)(rows->n / 4), n_peers = (uint32_t)(kp->n / sizeof(wgcs_keypairs));
      auto* const p = (wgcs_aead_pkt*)pkts->p;
      const auto* const kpr = (const uint32_t*)key_peer->p;
      const auto* const pr = (const uint32_t*)rows->p;
      const auto* const k = (const wgcs_keypairs*)kp->p;
      if (host) {
        if (wgcs_rekey_recv_gate_host(p, n, now, kpr, n_keys, pr, n_ids, k, n_peers) != 0) return 3;
      } else {
        each(RekeyRecvGate{{p, kpr, n_keys, pr, n_ids, n_peers}, now, k, p}, n);
      }
      outs = {pkts};
    } else if (op == "gate" || op == "sent") {
      const bool gate = op == "gate";
      const size_t b = gate ? 3 : 4;  // the fields in front of max_segs
      uint32_t max_segs = 0;
      uint64_t limit = 0;
      if (f.size() != b + 7 || f[1].size() % 4 || f[2].size() != f[1].size() || (!gate && f[3].size() != f[1].size()) ||
          !scalar(f[b], &max_segs) || f[0].size() != f[1].size() * max_segs || !scalar(f[b + 1], &now) ||
          f[b + 2].size() % 4 || f[b + 3].size() % sizeof(wgcs_keypairs) || f[b + 4].size() % 8 ||
          !scalar(f[b + 5], &limit) || f[b + 6].size() != f[b + 3].size() / sizeof(wgcs_keypairs) * sizeof(wgcs_rekey))
        return 2;
      const Exact *peer = exact(f[0]), *count = exact(f[1]), *status = exact(f[2]);
      const Exact* const job_key = gate ? nullptr : exact(f[3]);
      const Exact *rows = exact(f[b + 2]), *kp = exact(f[b + 3]), *nonce = exact(f[b + 4]), *rekey = exact(f[b + 6]);
      const uint32_t n = (uint32_t)(count->n / 4), n_ids = (uint32_t)(rows->n / 4);
      const uint32_t n_peers = (uint32_t)(kp->n / sizeof(wgcs_keypairs)), n_keys = (uint32_t)(nonce->n / 8);
      const auto* const pe = (const uint32_t*)peer->p;
      const auto* const c = (const int32_t*)count->p;
      const auto* const st = (const int32_t*)status->p;
      const auto* const pr = (const uint32_t*)rows->p;
      const auto* const k = (const wgcs_keypairs*)kp->p;
      const auto* const sn = (const uint64_t*)nonce->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      if (gate) {
        const Exact* const out = exact(filled(4 * (size_t)n));
        auto* const so = (int32_t*)out->p;
        if (host) {
          if (wgcs_rekey_send_gate_host(pe, c, st, n, max_segs, now, pr, n_ids, k, n_peers, sn, n_keys, limit, rk, so) != 0)
            return 3;
        } else {
          each(RekeySendGate{{pe, c, st, max_segs, pr, n_ids, n_peers}, now, k, sn, n_keys, limit, rk, so}, n);
        }
        outs = {out, rekey};
      } else {
        const auto* const jk = (const uint32_t*)job_key->p;
        if (host) {
          if (wgcs_rekey_sent_host(pe, c, st, jk, n, max_segs, now, pr, n_ids, k, n_peers, sn, n_keys, limit, rk) != 0)
            return 3;
        } else {
          each(RekeySent{{pe, c, st, max_segs, pr, n_ids, n_peers}, jk, now, k, sn, n_keys, limit, rk}, n);
        }
        outs = {rekey};
      }
    } else if (op == "rcvd") {
      uint32_t cpb = 0;
      if (f.size() != 6 || f[0].size() % sizeof(wgcs_write_group) || !scalar(f[1], &cpb) || cpb == 0 ||
          !scalar(f[2], &now) || f[3].size() % 4 || f[4].size() % sizeof(wgcs_keypairs) ||
          f[5].size() != f[4].size() / sizeof(wgcs_keypairs) * sizeof(wgcs_rekey))
        return 2;
      const Exact *groups = exact(f[0]), *rows = exact(f[3]), *kp = exact(f[4]), *rekey = exact(f[5]);
      const uint32_t n = (uint32_t)(groups->n / sizeof(wgcs_write_group)), n_ids = (uint32_t)(rows->n / 4);
      const uint32_t n_peers = (uint32_t)(kp->n / sizeof(wgcs_keypairs));
      if (n % cpb) return 2;
      const auto* const g = (const wgcs_write_group*)groups->p;
      const auto* const pr = (const uint32_t*)rows->p;
      const auto* const k = (const wgcs_keypairs*)kp->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      if (host) {
        if (wgcs_rekey_received_host(g, n / cpb, cpb, now, pr, n_ids, k, n_peers, rk) != 0) return 3;
      } else {
        each(RekeyReceived{{g, pr, n_ids, n_peers}, now, k, rk}, n);
      }
      outs = {rekey};
    } else if (op == "resp") {
      if (f.size() != 4 || f[0].size() % sizeof(wgcs_hs_resp) || f[1].size() != f[0].size() / sizeof(wgcs_hs_resp) * 4 ||
          !scalar(f[2], &now) || f[3].size() % sizeof(wgcs_rekey))
        return 2;
      const Exact *resp = exact(f[0]), *gate = exact(f[1]), *rekey = exact(f[3]);
      const uint32_t n = (uint32_t)(resp->n / sizeof(wgcs_hs_resp)), n_peers = (uint32_t)(rekey->n / sizeof(wgcs_rekey));
      const auto* const r = (const wgcs_hs_resp*)resp->p;
      const auto* const g = (const int32_t*)gate->p;
      auto* const rk = (wgcs_rekey*)rekey->p;
      if (host) {
        if (wgcs_rekey_responded_host(r, g, n, now, rk, n_peers) != 0) return 3;
      } else {
        each(RekeyResponded{{r, g, n_peers}, now, rk}, n);
      }
      outs = {rekey};
    } else if (op == "start") {
      if (f.size() != 4 || !scalar(f[0], &now) || f[1].size() % sizeof(wgcs_rekey) ||
          f[2].size() != f[1].size() / sizeof(wgcs_rekey) * sizeof(wgcs_hs_peer) || f[3].size() % sizeof(wgcs_hs_start))
        return 2;
      const Exact *rekey = exact(f[1]), *peers = exact(f[2]), *tickets = exact(f[3]);
      const uint32_t n_peers = (uint32_t)(rekey->n / sizeof(wgcs_rekey));
      const uint32_t n_tickets = (uint32_t)(tickets->n / sizeof(wgcs_hs_start));
      const Exact *status = exact(filled(4 * (size_t)n_peers)), *reasons = exact(filled(4 * (size_t)n_peers));
      const Exact *start = exact(filled(sizeof(wgcs_hs_start) * (size_t)n_tickets));
      const Exact *start_peer = exact(filled(4 * (size_t)n_tickets)), *count = exact(filled(4));
      auto* const rk = (wgcs_rekey*)rekey->p;
      const auto* const hp = (const wgcs_hs_peer*)peers->p;
      const auto* const t = (const wgcs_hs_start*)tickets->p;
      auto* const st = (int32_t*)status->p;
      auto* const why = (uint32_t*)reasons->p;
      auto* const d = (wgcs_hs_start*)start->p;
      auto* const sp = (uint32_t*)start_peer->p;
      auto* const cn = (uint32_t*)count->p;
      if (host) {
        if (wgcs_rekey_start_host(now, rk, hp, n_peers, t, n_tickets, d, sp, cn, st, why) != 0) return 3;
      } else {
        for (uint32_t r = 0; r < n_peers; ++r) st[r] = rekey_start_verdict(r, now, rk, why);
        uint32_t rank = 0;
        for (uint32_t r = 0; r < n_peers; ++r)
          if (st[r] == WGCS_HS_STARTED) st[r] = rekey_start_commit(r, rank++, now, rk, hp, t, n_tickets, d, sp);
        *cn = rank < n_tickets ? rank : n_tickets;
        for (uint32_t k = *cn; k < n_tickets; ++k) rekey_start_tail(k, d, sp);
      }
      outs = {status, reasons, start, start_peer, count, rekey};
    } else {
      return 2;
    }
    for (size_t i = 0; i < outs.size(); ++i) {
      if (i) printf(" ");
      print_hex(*outs[i]);
    }
    printf("\n");
  }
  printf("rekey_host: ok\n");
  return 0;
}
