// wgcs_replay.h -- the anti-replay filter of replay/replay.go (RFC 6479) as one
// scalar function, shared by the host entry points (replay_api.cpp), the
// stand-alone sanitizer program of tests/replay_host/ and, as the statement
// that the wave form of replay_kernels.hip must reproduce, the device code.
//
// A filter is `last`, the highest accepted value, and a ring of 128 blocks of
// 64 bits: bit (v & 63) of ring[(v >> 6) & 127] says that v was seen, for the
// values of the 128 blocks that end with last's.  The window that still
// accepts is 127 blocks (8,128 values) behind last, so a block is always
// cleared before it is reused.  Any bytes are a filter as far as memory safety
// goes: every index is masked and the clear loop is capped at the ring's size.
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WGCS_REPLAY_HD __host__ __device__ inline
#else
#define WGCS_REPLAY_HD inline
#endif

namespace wgcs {

constexpr uint32_t kReplayBlockShift = 6;                                   // replay.go:6
constexpr uint64_t kReplayBlocks = 128;                                     // :10
constexpr uint64_t kReplayBitMask = 63, kReplayBlockMask = 127;             // :11-12
constexpr uint64_t kReplayWindow = (kReplayBlocks - 1) << kReplayBlockShift;  // :13, 8,128

static_assert(sizeof(wgcs_replay_filter) == 1032, "replay.Filter layout");

// Filter.Validate, replay.go:32-70
WGCS_REPLAY_HD bool wgcs_replay_validate_one(wgcs_replay_filter* f, uint64_t value, uint64_t limit) {
  if (value >= limit) return false;  // :35-37
  uint64_t block = value >> kReplayBlockShift;
  if (value > f->last) {  // :42-56: the window moves forward
    const uint64_t current = f->last >> kReplayBlockShift;
    uint64_t diff = block - current;
    if (diff > kReplayBlocks) diff = kReplayBlocks;  // a longer jump makes the whole ring stale
    for (uint64_t i = 1; i <= diff; ++i) f->ring[(current + i) & kReplayBlockMask] = 0;
    f->last = value;
  } else if (f->last - value > kReplayWindow) {  // :57-59: behind the window
    return false;
  }
  block &= kReplayBlockMask;
  const uint64_t bit = 1ull << (value & kReplayBitMask);
  const uint64_t old = f->ring[block];
  f->ring[block] = old | bit;
  return (old & bit) == 0;  // :66-69
}

}  // namespace wgcs
