// batch_plan_host.cpp -- wgcs_batch_plan.h (how wgcs_checksum_batches cuts its
// batch list into launches) as host code under AddressSanitizer + UBSan
// (tests/test_batch_plan_host.py builds and runs it; no GPU, no library).  The
// batch list, the table and the index list are heap blocks of exactly their
// size, so an entry written past the table is a sanitizer report.  Pointers in
// the lists are addresses in a made-up range and are never dereferenced.
//
// The model of this file's own does not compare ranges pair by pair as the
// header does: it keeps one owner per output byte of the open group, and a
// batch joins the group when every byte it writes is free or owned by a batch
// with the very same tuple.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../wireguard_amd/csrc/wgcs_batch_plan.h"

using namespace wgcs;

namespace {

long g_checks = 0;

#define CHECK(c)                                                               \
  do {                                                                         \
    ++g_checks;                                                                \
    if (!(c)) {                                                                \
      fprintf(stderr, "batch_plan_host: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

constexpr uintptr_t kOutBase = 0x100000;  // made-up device addresses
constexpr size_t kOutSpan = 1 << 20;
const uint32_t kSizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049};

struct ModelGroup {
  std::vector<uint32_t> idx;     // list indices of the non-empty members, ascending
  std::vector<uint32_t> blocks;  // blocks of each
  uint32_t next;                 // list index the following group starts at
};

uint32_t model_blocks(uint32_t n, uint32_t ppb, uint64_t cap) {
  uint64_t cap8 = cap - cap % 8;
  uint64_t b = 0;
  while (b * ppb < n) ++b;  // ceil(n / ppb)
  while (b % 8) ++b;
  return (uint32_t)(b < cap8 ? b : cap8);
}

bool same(const wgcs_batch& a, const wgcs_batch& b) {
  return a.arena == b.arena && a.pkts == b.pkts && a.initial == b.initial && a.out == b.out && a.n == b.n;
}

std::vector<ModelGroup> model(const wgcs_batch* bl, uint32_t nb, uint32_t w, uint32_t ppb, uint64_t cap) {
  std::vector<ModelGroup> gs;
  static std::vector<int32_t> owner(kOutSpan, -1);  // list index of the batch that owns the byte in the open group
  uint32_t k = 0;
  while (k < nb) {
    ModelGroup g;
    std::vector<uintptr_t> touched;
    for (; k < nb && g.idx.size() < 32; ++k) {
      if (bl[k].n == 0) continue;
      const uintptr_t o = (uintptr_t)bl[k].out - kOutBase;
      bool ok = true;
      for (uintptr_t a = o; a < o + (uintptr_t)bl[k].n * w && ok; ++a)
        ok = owner[a] < 0 || same(bl[owner[a]], bl[k]);
      if (!ok) break;
      for (uintptr_t a = o; a < o + (uintptr_t)bl[k].n * w; ++a) {
        if (owner[a] < 0) touched.push_back(a);
        owner[a] = (int32_t)k;
      }
      g.idx.push_back(k);
      g.blocks.push_back(model_blocks(bl[k].n, ppb, cap));
    }
    g.next = k;
    for (uintptr_t a : touched) owner[a] = -1;
    gs.push_back(g);
  }
  return gs;
}

void check_list(const std::vector<wgcs_batch>& list, int mode, const BatchPlanCfg& cfg) {
  const uint32_t nb = (uint32_t)list.size();
  const uint32_t w = mode == WGCS_MODE_VALIDATE ? 1 : 2;
  CHECK(batch_out_width(mode) == w);
  wgcs_batch* bl = (wgcs_batch*)malloc(nb ? nb * sizeof(wgcs_batch) : 1);  // exactly nb rows
  if (nb) memcpy(bl, list.data(), nb * sizeof(wgcs_batch));
  const std::vector<ModelGroup> want = model(bl, nb, w, cfg.pkts_per_block, cfg.cap);
  BatchTable* tab = (BatchTable*)malloc(sizeof(BatchTable));
  uint32_t* idx = (uint32_t*)malloc(kBatchGroupMax * sizeof(uint32_t));
  std::vector<uint32_t> seen;
  size_t g = 0;
  for (uint32_t k = 0; k < nb; ++g) {
    memset(tab, 0xA5, sizeof *tab);
    memset(idx, 0xA5, kBatchGroupMax * sizeof(uint32_t));
    const uint32_t k1 = batch_plan_next(bl, nb, k, mode, cfg, tab, idx);
    CHECK(g < want.size());
    const ModelGroup& m = want[g];
    CHECK(k1 == m.next && k1 > k);  // group boundaries, and progress
    CHECK(tab->count == m.idx.size() && tab->count <= kBatchGroupMax);
    uint32_t total = 0;
    bool pow2_same = tab->count > 0;
    for (uint32_t e = 0; e < tab->count; ++e) {
      const wgcs_batch& b = bl[idx[e]];
      const BatchEntry& t = tab->e[e];
      CHECK(idx[e] == m.idx[e] && idx[e] >= k && idx[e] < k1 && b.n != 0);
      CHECK(t.arena == b.arena && t.pkts == b.pkts && t.initial == b.initial && t.out == b.out && t.n == b.n);
      CHECK(t.blocks == m.blocks[e] && t.blocks % 8 == 0 && t.blocks >= 8);
      CHECK(t.blocks <= cfg.cap);
      if (t.blocks < (cfg.cap & ~7ull)) CHECK((uint64_t)t.blocks * cfg.pkts_per_block >= b.n);  // one pass unless capped
      CHECK(t.first == total && tab->first[e] == total && total % 8 == 0);  // prefix sums
      total += t.blocks;
      pow2_same = pow2_same && t.blocks == tab->e[0].blocks && (t.blocks & (t.blocks - 1)) == 0;
      seen.push_back(idx[e]);
    }
    CHECK(tab->total == total);
    for (uint32_t e = tab->count; e < kBatchGroupMax; ++e)
      CHECK(tab->first[e] == kBatchNoEntry && tab->e[e].n == 0 && tab->e[e].blocks == 0);
    if (pow2_same) CHECK(tab->same_shift < 32 && (1u << tab->same_shift) == tab->e[0].blocks);
    else CHECK(tab->same_shift == kBatchNoEntry);
    // the lookup the kernel does, on every 8th block and both ends of every entry
    for (uint32_t e = 0; e < tab->count; ++e)
      for (uint32_t bi = tab->first[e]; bi < tab->first[e] + tab->e[e].blocks; bi += 8)
        for (uint32_t x : {bi, bi + 7}) {
          uint32_t got = 0;
          if (tab->same_shift != kBatchNoEntry) got = x >> tab->same_shift;
          else
            for (uint32_t q = 1; q < kBatchGroupMax; ++q) got = x >= tab->first[q] ? q : got;
          CHECK(got == e);
        }
    k = k1;
  }
  CHECK(g == want.size());
  // every non-empty batch exactly once and in order
  std::vector<uint32_t> nonempty;
  for (uint32_t k = 0; k < nb; ++k)
    if (bl[k].n) nonempty.push_back(k);
  CHECK(seen == nonempty);
  free(idx);
  free(tab);
  free(bl);
}

std::vector<wgcs_batch> random_list(std::mt19937& rng, uint32_t nb, uint32_t w, int flavour) {
  std::vector<wgcs_batch> l;
  uintptr_t fresh = kOutBase;
  auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
  for (uint32_t k = 0; k < nb; ++k) {
    wgcs_batch b;
    memset(&b, 0, sizeof b);
    b.n = kSizes[pick(8)];
    if (flavour == 2) b.n = pick(4) ? b.n : 0;  // many empty batches, adjacent ones too
    b.arena = (uint8_t*)(uintptr_t)(0x10000000u + 0x1000u * pick(4));
    b.pkts = (const wgcs_pkt*)(uintptr_t)(0x20000000u + 0x1000u * pick(4));
    b.initial = pick(2) ? (const uint64_t*)(uintptr_t)(0x30000000u + 0x1000u * pick(2)) : nullptr;
    const uint32_t kind = flavour == 0 ? 0 : pick(8);  // flavour 0: all disjoint
    const wgcs_batch* prev = l.empty() ? nullptr : &l[pick((uint32_t)l.size())];
    uintptr_t out = 0;
    if (prev && prev->n && kind == 1) {  // the identical tuple (the benchmark's rotation)
      b = *prev;
      out = (uintptr_t)b.out;
    } else if (prev && prev->n && kind == 2) {  // partial overlap: starts inside the earlier range, ends past it
      out = (uintptr_t)prev->out + (uintptr_t)prev->n * w / 2;
    } else if (prev && prev->n > 2 && kind == 3) {  // nested
      out = (uintptr_t)prev->out + w;
      b.n = b.n < prev->n - 2 ? b.n : prev->n - 2;
    } else if (prev && prev->n && kind == 4) {  // the same range for other packets
      out = (uintptr_t)prev->out;
      b.n = prev->n;
      b.pkts = (const wgcs_pkt*)((uintptr_t)prev->pkts + 16);
    } else if (prev && prev->n && kind == 5) {  // abutting: ends where the earlier range starts, or starts at its end
      out = (uintptr_t)prev->out + (uintptr_t)prev->n * w;
    } else {
      out = fresh;
    }
    b.out = (void*)out;
    const uintptr_t end = out + (uintptr_t)b.n * w;
    if (end > fresh) fresh = end + pick(3);
    CHECK(fresh < kOutBase + kOutSpan - 8192);
    l.push_back(b);
  }
  return l;
}

}  // namespace

int main() {
  // the switch, as wgcs_init reads it
  const bool fuse = batch_plan_fuse_env(getenv("WGCS_FUSE"));
  CHECK(batch_plan_fuse_env(nullptr) && batch_plan_fuse_env("1") && !batch_plan_fuse_env("0") &&
        batch_plan_fuse_env("2"));
  const BatchPlanCfg cfgs[] = {{8, 256ull * 1024, fuse}, {8, 256, fuse}, {8, 8, fuse},  {4, 20, fuse},
                               {16, 100, fuse},          {8, 7, fuse},   {8, 0, fuse},  {8, 1ull << 40, fuse}};
  std::mt19937 rng(20240611);
  long lists = 0;
  for (const BatchPlanCfg& cfg : cfgs) {
    const bool room = (cfg.cap & ~7ull) >= 8;
    CHECK(batch_plan_fusable(0, cfg) == (fuse && room));
    CHECK(!batch_plan_fusable(WGCS_F_INPLACE, cfg));  // INPLACE keeps its per-batch launches
    BatchPlanCfg off = cfg;
    off.fuse = false;
    CHECK(!batch_plan_fusable(0, off));
    if (!room) continue;  // no groups are made: nothing to plan
    BatchPlanCfg on = cfg;
    on.fuse = true;  // the cutting rule itself does not depend on the switch
    for (int mode : {WGCS_MODE_FOLD, WGCS_MODE_L4_FILL, WGCS_MODE_VALIDATE, WGCS_MODE_PARTIAL, WGCS_MODE_IP4HDR}) {
      const uint32_t w = mode == WGCS_MODE_VALIDATE ? 1 : 2;
      for (int flavour = 0; flavour < 3; ++flavour)
        for (int rep = 0; rep < 12; ++rep, ++lists) {
          const uint32_t nb = rep == 0 ? 0 : rep == 1 ? 1 : rep == 2 ? 100 : (uint32_t)(rng() % 101);
          check_list(random_list(rng, nb, w, flavour), mode, on);
        }
      // 70 equal disjoint batches (32 + 32 + 6), and all-empty lists
      std::vector<wgcs_batch> eq;
      for (uint32_t k = 0; k < 70; ++k) {
        wgcs_batch b;
        memset(&b, 0, sizeof b);
        b.arena = (uint8_t*)(uintptr_t)0x10000000u;
        b.pkts = (const wgcs_pkt*)(uintptr_t)0x20000000u;
        b.out = (void*)(kOutBase + (uintptr_t)k * 4096);
        b.n = 2048;
        eq.push_back(b);
      }
      check_list(eq, mode, on);
      for (wgcs_batch& b : eq) b.n = 0;
      check_list(eq, mode, on);
    }
  }
  printf("%ld lists, %ld checks\nbatch_plan_host: ok\n", lists, g_checks);
  return 0;
}
