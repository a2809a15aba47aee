// write_host.cpp -- wgcs_write_plan.h's scalar rule as host code under
// AddressSanitizer + UBSan (tests/test_write_host.py builds and runs it; no
// GPU, no library).  Every input and output array is a heap block of exactly
// its size, so a row written or read past a batch's share of a table's last
// batch is a sanitizer report, and every output starts as a marker, so a row
// the rule leaves out shows as a difference.
//
// The model of this file's own does not walk the rows the way the header
// does: it sorts (peer, row) pairs, cuts the sorted list into one run per
// peer, orders the runs by their first row, and builds each table from the
// runs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../../wireguard_amd/csrc/wgcs_write_plan.h"

namespace {

int g_checks = 0;

#define CHECK(c)                                                          \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(c)) {                                                           \
      fprintf(stderr, "write_host: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

template <typename T>
T* heap(size_t n, int fill) {  // exactly n rows
  T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
  memset(p, fill, n * sizeof(T));
  return p;
}

struct Tables {
  std::vector<wgcs_gro_buf> bufs;
  std::vector<wgcs_gro_call> calls;
  std::vector<wgcs_write_group> groups;
  std::vector<int32_t> n_groups, status;
};

bool takes_part(int32_t v) { return v >= 0 || v == -19 || v == -8; }  // SOURCE, PACKET_TOO_SHORT

Tables model(const wgcs_aead_pkt* pk, const int32_t* vd, uint32_t n_msgs, uint32_t nb, const uint32_t* key_peer,
             uint32_t n_keys, int32_t offset, uint32_t cap, uint32_t flags, uint32_t cpb) {
  Tables t;
  t.bufs.assign((size_t)nb * n_msgs, wgcs_gro_buf{0, 0, 0});
  t.calls.resize((size_t)nb * cpb);
  t.groups.assign((size_t)nb * cpb, wgcs_write_group{0xFFFFFFFFu, -1, 0, 0, 0});
  t.n_groups.resize(nb);
  t.status.resize(nb);
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t q0 = b * n_msgs;
    for (uint32_t g = 0; g < cpb; ++g) t.calls[(size_t)b * cpb + g] = wgcs_gro_call{q0, 0, offset, flags};
    std::vector<std::pair<uint32_t, uint32_t>> rows;  // (peer, q)
    bool panic = false;
    for (uint32_t q = q0; q < q0 + n_msgs; ++q) {
      if (pk[q].key >= n_keys || key_peer[pk[q].key] == 0xFFFFFFFFu || !takes_part(vd[q])) continue;
      rows.push_back({key_peer[pk[q].key], q});
      if (vd[q] > 0 && (long long)offset + vd[q] > (long long)cap) panic = true;
    }
    std::sort(rows.begin(), rows.end());
    std::vector<std::vector<uint32_t>> runs;  // per peer, rows ascending
    for (size_t i = 0; i < rows.size(); ++i) {
      if (i == 0 || rows[i].first != rows[i - 1].first) runs.emplace_back();
      runs.back().push_back(rows[i].second);
    }
    std::sort(runs.begin(), runs.end(), [](const auto& a, const auto& c) { return a[0] < c[0]; });
    t.n_groups[b] = (int32_t)runs.size();
    t.status[b] = panic ? -13 : runs.size() > cpb ? -14 : 0;
    if (t.status[b]) continue;
    uint32_t at = q0;
    for (size_t g = 0; g < runs.size(); ++g) {
      wgcs_write_group w{key_peer[pk[runs[g][0]].key], (int32_t)runs[g].back(), 0, (uint32_t)runs[g].size(), 0};
      const uint32_t first = at;
      for (uint32_t q : runs[g]) {
        w.rx_bytes += pk[q].len;
        if (pk[q].len > 32) w.flags = WGCS_GROUP_DATA;
        if (vd[q] > 0) t.bufs[at++] = wgcs_gro_buf{pk[q].off, (uint32_t)(offset + vd[q]), cap};
      }
      t.groups[(size_t)b * cpb + g] = w;
      t.calls[(size_t)b * cpb + g] = wgcs_gro_call{first, at - first, offset, flags};
    }
  }
  return t;
}

struct Counts {
  int batches = 0, multi = 0, empty_call = 0, none = 0, full = 0, range = 0, all_kept = 0;
};

void run_table(std::mt19937_64& rng, uint32_t n_msgs, uint32_t cpb, uint32_t nb, Counts& seen) {
  auto pick = [&](uint64_t n) { return (uint32_t)(rng() % n); };
  const uint32_t n_keys = 1 + pick(140), n = n_msgs * nb;
  const int32_t offset = (int32_t)pick(3) * 16;
  const uint32_t cap = (uint32_t)offset + 1 + pick(2000), flags = pick(2);
  uint32_t* key_peer = heap<uint32_t>(n_keys, 0);
  const uint32_t n_peers = 1 + pick(n_keys);
  for (uint32_t k = 0; k < n_keys; ++k) key_peer[k] = pick(12) == 0 ? 0xFFFFFFFFu : 1000 + pick(n_peers);
  wgcs_aead_pkt* pk = heap<wgcs_aead_pkt>(n, 0);
  int32_t* vd = heap<int32_t>(n, 0);
  static const int32_t codes[] = {0, -1, -8, -13, -18, -19, -20};
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t spread = 1 + pick(pick(2) ? n_keys : 3), err = pick(3), full = pick(8) == 0;
    for (uint32_t q = b * n_msgs; q < (b + 1) * n_msgs; ++q) {
      pk[q].off = rng() >> 16;
      pk[q].counter = rng();
      pk[q].key = full ? q % (n_keys < 2 ? n_keys : 2) : pick(20) == 0 ? (pick(2) ? 0xFFFFFFFFu : n_keys) : pick(spread);
      pk[q].len = pick(50) == 0 ? 0xFFFFFFFFu - pick(4) : 32 + pick(3) * pick(1400);
      vd[q] = !full && pick(3) < err ? codes[pick(7)] : 1 + (int32_t)pick(cap - offset);
      if (pick(400) == 0) vd[q] = (int32_t)(cap - offset) + 1 + (int32_t)pick(50);
    }
  }
  wgcs_gro_buf* bufs = heap<wgcs_gro_buf>(n, 0xC7);
  wgcs_gro_call* calls = heap<wgcs_gro_call>((size_t)nb * cpb, 0xC7);
  wgcs_write_group* groups = heap<wgcs_write_group>((size_t)nb * cpb, 0xC7);
  int32_t* n_groups = heap<int32_t>(nb, 0xC7);
  int32_t* status = heap<int32_t>(nb, 0xC7);
  CHECK(wgcs::write_args_ok(n_msgs, nb, offset, cap, cpb));
  // batches in descending order: a batch touches its own rows only
  for (uint32_t b = nb; b-- > 0;)
    status[b] = wgcs::write_plan_batch(pk, vd, b, n_msgs, key_peer, n_keys, offset, cap, flags, cpb, bufs, calls,
                                       groups, n_groups + b);
  const Tables want = model(pk, vd, n_msgs, nb, key_peer, n_keys, offset, cap, flags, cpb);
  CHECK(memcmp(bufs, want.bufs.data(), n * sizeof *bufs) == 0);
  CHECK(memcmp(calls, want.calls.data(), (size_t)nb * cpb * sizeof *calls) == 0);
  CHECK(memcmp(groups, want.groups.data(), (size_t)nb * cpb * sizeof *groups) == 0);
  CHECK(memcmp(n_groups, want.n_groups.data(), nb * sizeof(int32_t)) == 0);
  CHECK(memcmp(status, want.status.data(), nb * sizeof(int32_t)) == 0);
  for (uint32_t b = 0; b < nb; ++b) {
    ++seen.batches;
    seen.none += n_groups[b] == 0;
    seen.full += status[b] == -14;
    seen.range += status[b] == -13;
    if (status[b]) continue;
    seen.multi += n_groups[b] > 1;
    uint32_t kept = 0;
    for (int32_t g = 0; g < n_groups[b]; ++g) {
      seen.empty_call += calls[(size_t)b * cpb + g].n == 0;
      kept += calls[(size_t)b * cpb + g].n;
    }
    seen.all_kept += kept == n_msgs && n_msgs == 128;
  }
  free(key_peer), free(pk), free(vd), free(bufs), free(calls), free(groups), free(n_groups), free(status);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  static const uint32_t sizes[] = {1, 2, 3, 63, 64, 65, 127, 128};
  Counts seen;
  for (int round = 0; round < 60; ++round)
    for (uint32_t n_msgs : sizes)
      for (uint32_t cpb : {1u, 2u, n_msgs / 2, n_msgs})
        if (cpb >= 1 && cpb <= n_msgs) run_table(rng, n_msgs, cpb, 1 + (uint32_t)(rng() % 5), seen);
  CHECK(seen.batches >= 3000);
  CHECK(seen.multi && seen.empty_call && seen.none && seen.full && seen.range && seen.all_kept);
  // the scalar argument rule
  CHECK(!wgcs::write_args_ok(0, 1, 0, 0, 1) && !wgcs::write_args_ok(129, 1, 0, 0, 1));
  CHECK(!wgcs::write_args_ok(4, 1, 0, 0, 0) && !wgcs::write_args_ok(4, 1, 0, 0, 5));
  CHECK(!wgcs::write_args_ok(4, 1, -1, 0, 1) && !wgcs::write_args_ok(4, 1, 17, 16, 1));
  CHECK(!wgcs::write_args_ok(128, (1u << 21) + 1, 0, 0, 1) && wgcs::write_args_ok(128, 1u << 21, 16, 16, 128));
  CHECK(wgcs::write_args_ok(1, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 1) == false);
  printf("%d checks, %d batches\nwrite_host: ok\n", g_checks, seen.batches);
  return 0;
}
