// replay_host.cpp -- wgcs_replay.h's scalar filter as host code under
// AddressSanitizer + UBSan (tests/test_replay_host.py builds and runs it; no
// GPU, no library).  Every filter lives in a heap block of exactly
// sizeof(wgcs_replay_filter) = 1,032 bytes, so an index that leaves the ring
// is a sanitizer report.  Filters start all-zero, all-ones and random: any
// bytes are a filter as far as memory safety goes.
//
// Two models of this file's own check the verdicts:
//   Bits   one flag per value of the 8,192-value ring, `last`, and the window
//          moved value by value; it starts from any filter's bytes
//   Seen   a std::set of accepted values and their maximum; it is the meaning
//          of a filter that started empty
// and after every sequence the filter's bytes must be what Bits holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../wireguard_amd/csrc/wgcs_replay.h"

namespace {

constexpr uint64_t kRing = 8192, kWindow = 8128;
int g_checks = 0;

#define CHECK(c)                                                      \
  do {                                                                \
    ++g_checks;                                                       \
    if (!(c)) {                                                       \
      fprintf(stderr, "replay_host: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct Bits {
  uint64_t last;
  std::vector<bool> seen = std::vector<bool>(kRing);
  explicit Bits(const wgcs_replay_filter* f) : last(f->last) {
    for (uint64_t x = 0; x < kRing; ++x) seen[x] = (f->ring[x >> 6] >> (x & 63)) & 1;
  }
  bool validate(uint64_t v, uint64_t limit) {
    if (v >= limit) return false;
    if (v > last) {
      // every value of the blocks after last's, up to v's block, leaves the ring; 8,192 of them are all there are
      const uint64_t from = (last | 63) + 1;  // last < v <= 2^64 - 2: no wrap unless v is in last's block
      if ((v >> 6) > (last >> 6)) {
        const uint64_t to = v | 63;  // inclusive
        const uint64_t count = to - from + 1 > kRing || to - from + 1 == 0 ? kRing : to - from + 1;
        for (uint64_t i = 0; i < count; ++i) seen[(from + i) % kRing] = false;
      }
      last = v;
    } else if (last - v > kWindow) {
      return false;
    }
    const bool was = seen[v % kRing];
    seen[v % kRing] = true;
    return !was;
  }
  bool equals(const wgcs_replay_filter* f) const {
    if (f->last != last) return false;
    for (uint64_t x = 0; x < kRing; ++x)
      if (seen[x] != (bool)((f->ring[x >> 6] >> (x & 63)) & 1)) return false;
    return true;
  }
};

struct Seen {
  uint64_t last = 0;
  std::set<uint64_t> seen;
  bool validate(uint64_t v, uint64_t limit) {
    if (v >= limit) return false;
    if (v <= last && last - v > kWindow) return false;
    if (v > last) last = v;
    return seen.insert(v).second;
  }
};

wgcs_replay_filter* fresh(int kind, std::mt19937_64& rng) {
  auto* f = (wgcs_replay_filter*)malloc(sizeof(wgcs_replay_filter));  // exactly 1,032 bytes
  if (!f) exit(2);
  if (kind == 0) {
    memset(f, 0, sizeof *f);
  } else if (kind == 1) {
    memset(f, 0xFF, sizeof *f);
  } else {
    f->last = (rng() & 3) ? rng() >> (rng() % 64) : rng();
    for (auto& w : f->ring) w = rng();
  }
  return f;
}

uint64_t next_value(std::mt19937_64& rng, uint64_t& cur, uint64_t limit, const std::vector<uint64_t>& hist) {
  const unsigned r = rng() % 100;
  if (r < 50) return cur += 1 + rng() % 3;
  if (r < 60 && !hist.empty()) return hist[hist.size() - 1 - rng() % (hist.size() < 70 ? hist.size() : 70)];
  if (r < 70) return cur - (rng() % 200 < cur ? rng() % 200 : 0);
  if (r < 80) return cur >= kWindow + 3 ? cur - kWindow - 3 + rng() % 7 : cur;
  if (r < 90) {
    static const uint64_t jumps[] = {63, 64, 65, 127 * 64, 128 * 64 - 1, 128 * 64, 128 * 64 + 1, 300 * 64, 1ull << 40};
    return cur += jumps[rng() % 9];
  }
  if (r < 94) return limit - 2 + rng() % 5;  // wraps around 0 for tiny limits: still a value
  if (r < 97) return ~0ull - rng() % 3;
  return rng();
}

void run_sequences(std::mt19937_64& rng) {
  for (int kind = 0; kind < 3; ++kind) {
    for (int seq = 0; seq < 300; ++seq) {
      wgcs_replay_filter* f = fresh(kind, rng);
      Bits bits(f);
      Seen seen;
      const uint64_t limit = (rng() % 4) ? WGCS_REJECT_AFTER_MESSAGES : (rng() % 3 ? 1 + rng() % (1u << 20) : ~0ull);
      uint64_t cur = kind == 0 ? (rng() % 2) * (rng() >> 30) : f->last;
      std::vector<uint64_t> hist;
      const int n = 1 + rng() % 500;
      for (int i = 0; i < n; ++i) {
        const uint64_t v = next_value(rng, cur, limit, hist);
        hist.push_back(v);
        const bool got = wgcs::wgcs_replay_validate_one(f, v, limit);
        CHECK(got == bits.validate(v, limit));
        if (kind == 0) CHECK(got == seen.validate(v, limit));
        if (v < limit && v > cur) cur = v;
      }
      CHECK(bits.equals(f));
      free(f);
    }
  }
}

void run_edges() {
  std::mt19937_64 rng(1);
  const uint64_t lim = WGCS_REJECT_AFTER_MESSAGES;
  struct Case {
    std::vector<uint64_t> v;
    std::vector<int> want;
  };
  const Case cases[] = {
      {{0, 0}, {1, 0}},
      {{8128 + 5, 5, 5}, {1, 1, 0}},
      {{8128 + 6, 5}, {1, 0}},
      {{lim - 1, lim, lim + 1, ~0ull, lim - 1}, {1, 0, 0, 0, 0}},
      {{1, 64, 1, 64}, {1, 1, 0, 0}},
      {{1, 65, 1, 65}, {1, 1, 0, 0}},
      {{1, 1 + 127 * 64, 1, 2}, {1, 1, 0, 1}},
      {{1, 1 + 128 * 64, 1}, {1, 1, 0}},
      {{7, 7 + (1ull << 40), 7, 7 + (1ull << 40) - 8128, 7 + (1ull << 40) - 8129}, {1, 1, 0, 1, 0}},
      {{100, 100 + 200 * 64, 100 + 8192, 100 + 8192, 100}, {1, 1, 1, 0, 0}},
  };
  for (const Case& c : cases) {
    wgcs_replay_filter* f = fresh(0, rng);
    for (size_t i = 0; i < c.v.size(); ++i) CHECK((int)wgcs::wgcs_replay_validate_one(f, c.v[i], lim) == c.want[i]);
    free(f);
  }
  // limit 0 accepts nothing and writes nothing
  wgcs_replay_filter* f = fresh(1, rng);
  CHECK(!wgcs::wgcs_replay_validate_one(f, 0, 0) && f->last == ~0ull);
  free(f);
}

}  // namespace

int main() {
  static_assert(sizeof(wgcs_replay_filter) == 1032 && alignof(wgcs_replay_filter) == 8, "layout");
  std::mt19937_64 rng(20261020);
  run_edges();
  run_sequences(rng);
  printf("%d checks\nreplay_host: ok\n", g_checks);
  return 0;
}
