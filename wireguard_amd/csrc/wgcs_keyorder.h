// wgcs_keyorder.h -- key order (keyorder.hip): the rows of a batch grouped by
// key with slot order kept inside each key, the one primitive that the replay
// filter and the send-nonce assignment share (replay_kernels.hip).  Internal;
// not part of the ABI.
//
// The caller fills keys_in[i] with row i's key row, or n_keys for a row that
// does not take part; keyorder_sort leaves
//   keys[p], slots[p]   the rows in (key, slot) order, the n_keys ones last
//   heads[0 .. *n_heads)  the position p of the first row of every key < n_keys
//                       that has one, in no particular order
// A segment ends where keys[p] changes or at n: whoever walks it reads the
// keys as it goes, so nothing here is sized by n_keys.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace wgcs {

constexpr uint32_t kKeyOrderMaxRows = 1u << 24, kKeyOrderMaxKeys = 1u << 24;

struct KeyOrder {
  uint32_t *keys_in, *slots_in;  // filled by the caller's own kernel (slots_in[i] = i)
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

}  // namespace wgcs
