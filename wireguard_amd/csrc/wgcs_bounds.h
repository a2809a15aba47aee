// wgcs_bounds.h -- the row bounds that the entry points check, the slot-count rule, and the overlap
// test of two caller ranges.  No HIP types: the *_api.cpp files (through wgcs_ctx.h) and the host
// forms, which the sanitizer programs of tests/*_host build as plain C++, include this one text.
#pragma once

#include <stdint.h>

namespace wgcs {

// what the key order (wgcs_keyorder.h) sorts in one call: its rows, and the key rows they name
constexpr uint32_t kKeyOrderMaxRows = 1u << 24, kKeyOrderMaxKeys = 1u << 24;

constexpr uint32_t kMaxRows = 1u << 28;           // rows of a batch or a table: counted in 32 bits, a pitch included
constexpr uint32_t kMaxPeers = kKeyOrderMaxKeys;  // rows of a per-peer table: a key space of the key order

// a table size the slot hash can mask
inline bool pow2_or_0(uint32_t n) { return (n & (n - 1)) == 0; }

// [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

}  // namespace wgcs
