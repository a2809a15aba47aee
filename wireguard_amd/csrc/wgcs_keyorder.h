// wgcs_keyorder.h -- key order (keyorder.hip): the rows of a batch grouped by key with slot order kept
// inside each key, and the walk over a key's rows.  Six calls rest on it; their kernel
// files keep the row logic.  Internal; not part of the ABI.
//
// The caller's keys kernel fills keys_in[i] with row i's key row, or n_keys for a row that does not take
// part (keyorder_put); keyorder_sort leaves
//   keys[p], slots[p]     the rows in (key, slot) order, the n_keys ones last
//   heads[0 .. *n_heads)  the position of the first row of every key < n_keys that has one, in no order
// A segment ends where keys[p] changes or at n: whoever walks it reads the keys as it goes, so nothing
// here is sized by n_keys.  The walk (the __HIPCC__ section) has two forms:
//   a wave per segment   KeySegments deals the segments heads[wave], heads[wave + n_waves], ... and
//       its trips() takes one 64 rows at a trip, lane l at position p + l.  The order is sorted by key,
//       so the rows of a trip are a prefix of the lanes: m rows are lanes 0 .. m - 1, and m < 64 is the
//       same as ~ballot != 0.  Such a trip is the segment's last.  A segment that fills its last trip
//       exactly costs one more trip with m == 0, which runs no body: the body sees 1 <= m <= 64.
//   a lane per segment   KeyRun, row by row, where segments are short and the row function is long.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "wgcs_bounds.h"  // kKeyOrderMaxRows, kKeyOrderMaxKeys
#include "wgcs_wave.h"

namespace wgcs {

struct KeyOrder {
  uint32_t *keys_in, *slots_in;  // filled by the caller's own kernel (keyorder_put)
  uint32_t *keys, *slots;        // sorted
  uint32_t *heads, *n_heads;     // n_heads leads 256 bytes of its own: the words behind it are the caller's
                                 // (stage: the count of staged jobs), and keyorder_sort zeroes *n_heads alone
  uint64_t* base;                // n words for the caller (send assign: a job's first nonce)
  void* sort_tmp;
  size_t sort_tmp_bytes;
};

// an upper bound of what keyorder_carve + the sort need for n rows
size_t keyorder_work_bytes(uint32_t n);
// false: work_bytes is too small for the arrays above (d_work is 16-byte aligned)
bool keyorder_carve(void* d_work, size_t work_bytes, uint32_t n, KeyOrder* ko);
// *fits = the sort's own temporary storage for (n, n_keys) fits ko.sort_tmp_bytes; launches nothing
hipError_t keyorder_check(const KeyOrder& ko, uint32_t n, uint32_t n_keys, hipStream_t s, bool* fits);
// the stable sort on ceil(log2(n_keys + 1)) bits, then the heads
hipError_t keyorder_sort(const KeyOrder& ko, uint32_t n, uint32_t n_keys, hipStream_t s);

// The kernels around the sort run kKeyOrderThreads lanes a block.
constexpr int kKeyOrderThreads = 256, kKeyOrderWaves = kKeyOrderThreads / kWave;
constexpr uint32_t kKeyOrderMaxGroupBlocks = 2048;  // the wave walk strides over the segments

// the grid of a lane-per-row kernel over n rows
inline uint32_t keyorder_blocks(uint32_t n) { return (n + kKeyOrderThreads - 1) / kKeyOrderThreads; }
// the grid of a wave-per-segment kernel over n rows: a wave per segment, at most n of them
inline uint32_t keyorder_group_blocks(uint32_t n) {
  const uint32_t b = (n + kKeyOrderWaves - 1) / kKeyOrderWaves;
  return b < kKeyOrderMaxGroupBlocks ? b : kKeyOrderMaxGroupBlocks;
}

#ifdef __HIPCC__

// The tail of a keys kernel: row i's key (n_keys: it does not take part) and its slot.
__device__ inline void keyorder_put(uint32_t* __restrict__ keys_in, uint32_t* __restrict__ slots_in, uint32_t i,
                                    uint32_t key) {
  keys_in[i] = key;
  slots_in[i] = i;
}

// The segments of this wave in a grid of kKeyOrderThreads lanes a block, and the trips over one:
//   for (KeySegments seg(keys, heads, n_heads, n); seg.next();) {
//     ... seg.key ...
//     seg.trips(lane, [&](bool mine, uint64_t pos, int m) { ... });
//   }
// Every lane of the wave calls trips; trip(mine, pos, m) runs once per trip with: this lane holds a row,
// at position pos; m, wave-uniform, the rows of the trip.  (A callable and not an iterator with a next():
// that form kept its stop flag in registers over the body and cost assign 5 % with one key.)
struct KeySegments {
  const uint32_t *keys, *heads;
  uint32_t n, nh, h, n_waves;
  uint32_t p0, key;  // the segment: its first position and its key

  __device__ KeySegments(const uint32_t* keys_, const uint32_t* heads_, const uint32_t* n_heads, uint32_t n_)
      : keys(keys_), heads(heads_), n(n_), nh(*n_heads),  // <= n
        h(__builtin_amdgcn_readfirstlane(blockIdx.x * kKeyOrderWaves + threadIdx.x / kWave)),
        n_waves(gridDim.x * kKeyOrderWaves), p0(0), key(0) {}

  __device__ bool next() {
    if (h >= nh) return false;
    p0 = heads[h];
    key = keys[p0];
    h += n_waves;
    return true;
  }
  template <typename Trip>
  __device__ void trips(uint32_t lane, Trip trip) const {
    for (uint64_t p = p0;; p += kWave) {
      const uint64_t pos = p + lane;
      const bool mine = pos < n && keys[pos] == key;
      const int m = __builtin_amdgcn_readfirstlane(__popcll(__ballot(mine)));
      if (m == 0) break;
      trip(mine, pos, m);
      if (m < kWave) break;
    }
  }
};

// The rows of the segment at heads[h], one lane, row by row (none if h is no segment):
//   for (KeyRun r(keys, heads, n_heads, n, h); r.more(); ++r.p) { slots[r.p] ... }
struct KeyRun {
  const uint32_t* keys;
  uint32_t n, key, p;

  __device__ KeyRun(const uint32_t* keys_, const uint32_t* heads, const uint32_t* n_heads, uint32_t n_, uint32_t h)
      : keys(keys_), n(n_), key(0), p(n_) {
    if (h < *n_heads) {  // <= n
      p = heads[h];
      key = keys[p];
    }
  }
  __device__ bool more() const { return p < n && keys[p] == key; }
};

#endif  // __HIPCC__

}  // namespace wgcs
