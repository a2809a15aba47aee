// wgcs_batch_plan.h -- how one wgcs_checksum_batches call is cut into launches:
// runs of consecutive batches ("groups") that one launch of the multi-batch
// checksum kernel processes concurrently, and the table that launch reads.
// Plain C++ and no HIP types, like wgcs_host.h: api.cpp, the kernel
// (checksum_kernels.hip) and the stand-alone sanitizer program of
// tests/batch_plan_host/ include the same header.
//
// Rules:
//  - a group holds at most kBatchGroupMax non-empty batches, in call order;
//    batches with n == 0 take no entry and no blocks;
//  - batch blocks: ceil(n / packets_per_block), rounded up to a multiple of 8,
//    capped at num_cu x blocks_per_cu rounded down to a multiple of 8 (the
//    kernel grid-strides beyond the cap); an entry's `first` is the prefix sum,
//    so every entry starts on a multiple of 8 and the XCD-aware block order of
//    the single-batch kernel holds inside each batch;
//  - two batches share a group only when running them concurrently cannot
//    change a result: their out ranges [out, out + n w) are disjoint, or they
//    are the same (arena, pkts, initial, out, n) tuple (both then write the
//    same bytes).  Any other overlap closes the group; groups run in order on
//    one stream, so the later batch's write still wins;
//  - nothing is deduplicated: every batch of the list is read and summed;
//  - WGCS_F_INPLACE (the kernel writes the arena, and batches k and k + S of a
//    call are ordered on one stream), fusing switched off (WGCS_FUSE=0) or a
//    cap below 8 blocks: no groups at all, the call keeps its per-batch
//    launches (batch_plan_fusable).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"

namespace wgcs {

constexpr uint32_t kBatchGroupMax = 32;
constexpr uint32_t kBatchNoEntry = 0xFFFFFFFFu;  // first[] of an unused entry: no block index reaches it

// One batch of a group as the kernel reads it (kernel-argument segment).
struct BatchEntry {
  uint8_t* arena;
  const wgcs_pkt* pkts;
  const uint64_t* initial;
  void* out;
  uint32_t n;
  uint32_t blocks;  // a multiple of 8
  uint32_t first;   // first block of the batch in the launch's grid (prefix sum, a multiple of 8)
  uint32_t pad;
};
struct BatchTable {
  uint32_t first[kBatchGroupMax];  // entry e's first block; kBatchNoEntry from `count` on
  BatchEntry e[kBatchGroupMax];
  uint32_t count;       // entries in use
  uint32_t total;       // blocks of the launch
  uint32_t same_shift;  // every entry has 1 << same_shift blocks: entry = block >> same_shift; else kBatchNoEntry
  uint32_t pad;
};
static_assert(sizeof(BatchEntry) == 48 && sizeof(BatchTable) == 128 + 32 * 48 + 16, "table layout");

struct BatchPlanCfg {
  uint32_t pkts_per_block;  // packets one block covers per grid-stride step
  uint64_t cap;             // num_cu x blocks_per_cu
  bool fuse;                // WGCS_FUSE
};

// WGCS_FUSE as wgcs_init reads it: unset or non-zero fuses
inline bool batch_plan_fuse_env(const char* v) {
  if (!v) return true;
  while (*v == ' ') ++v;
  return !(v[0] == '0' && v[1] == '\0');
}

inline uint32_t batch_out_width(int mode) { return mode == WGCS_MODE_VALIDATE ? 1u : 2u; }

// the cap as groups use it: rounded down to a multiple of 8, and small enough
// that a full group's block count stays far inside 31 bits
inline uint32_t batch_plan_cap8(const BatchPlanCfg& c) {
  const uint64_t lim = (uint64_t)0x7FFFFFF8u / kBatchGroupMax;
  const uint64_t cap = c.cap < lim ? c.cap : lim;
  return (uint32_t)(cap & ~(uint64_t)7);
}

inline bool batch_plan_fusable(unsigned flags, const BatchPlanCfg& c) {
  return c.fuse && !(flags & WGCS_F_INPLACE) && c.pkts_per_block > 0 && batch_plan_cap8(c) >= 8;
}

// blocks of a non-empty batch of n packets
inline uint32_t batch_plan_blocks(uint32_t n, const BatchPlanCfg& c) {
  uint64_t want = ((uint64_t)n + c.pkts_per_block - 1) / c.pkts_per_block;
  want = (want + 7) & ~(uint64_t)7;
  const uint32_t cap = batch_plan_cap8(c);
  return want < cap ? (uint32_t)want : cap;
}

inline bool batch_same_tuple(const wgcs_batch& a, const wgcs_batch& b) {
  return a.arena == b.arena && a.pkts == b.pkts && a.initial == b.initial && a.out == b.out && a.n == b.n;
}

// may batches a and b (both non-empty) run in one launch?
inline bool batch_may_share(const wgcs_batch& a, const wgcs_batch& b, uint32_t w) {
  const uintptr_t a0 = (uintptr_t)a.out, a1 = a0 + (uintptr_t)a.n * w;
  const uintptr_t b0 = (uintptr_t)b.out, b1 = b0 + (uintptr_t)b.n * w;
  return a1 <= b0 || b1 <= a0 || batch_same_tuple(a, b);
}

// The next group of a fusable call: starts at list index k0, fills *tab and
// idx[e] (the list index of entry e) and returns the list index the following
// group starts at (n_batches when the list is used up).  tab->count == 0 only
// when nothing but empty batches was left.
inline uint32_t batch_plan_next(const wgcs_batch* batches, uint32_t n_batches, uint32_t k0, int mode,
                                const BatchPlanCfg& c, BatchTable* tab, uint32_t* idx) {
  const uint32_t w = batch_out_width(mode);
  uint32_t cnt = 0, total = 0, k = k0;
  for (; k < n_batches && cnt < kBatchGroupMax; ++k) {
    const wgcs_batch& b = batches[k];
    if (b.n == 0) continue;
    bool ok = true;
    for (uint32_t e = 0; e < cnt && ok; ++e) ok = batch_may_share(batches[idx[e]], b, w);
    if (!ok) break;
    BatchEntry& t = tab->e[cnt];
    t.arena = b.arena;
    t.pkts = b.pkts;
    t.initial = b.initial;
    t.out = b.out;
    t.n = b.n;
    t.blocks = batch_plan_blocks(b.n, c);
    t.first = total;
    t.pad = 0;
    tab->first[cnt] = total;
    idx[cnt] = k;
    total += t.blocks;
    ++cnt;
  }
  for (uint32_t e = cnt; e < kBatchGroupMax; ++e) {
    tab->first[e] = kBatchNoEntry;
    tab->e[e] = BatchEntry{nullptr, nullptr, nullptr, nullptr, 0, 0, kBatchNoEntry, 0};
  }
  tab->count = cnt;
  tab->total = total;
  tab->same_shift = kBatchNoEntry;
  if (cnt) {
    const uint32_t nb = tab->e[0].blocks;
    bool same = (nb & (nb - 1)) == 0;
    for (uint32_t e = 1; e < cnt && same; ++e) same = tab->e[e].blocks == nb;
    if (same) {
      uint32_t s = 0;
      while ((1u << s) < nb) ++s;
      tab->same_shift = s;
    }
  }
  tab->pad = 0;
  return k;
}

}  // namespace wgcs
