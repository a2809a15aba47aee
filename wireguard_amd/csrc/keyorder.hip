// keyorder.hip -- key order (wgcs_keyorder.h): a stable radix sort of (key,
// slot) pairs on the bits a key row needs, and the first position of every
// key's segment.  The sort is rocPRIM's radix_sort_pairs (header-only; this is
// the one translation unit that includes it); the rest is plain HIP.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "wgcs_keyorder.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr size_t kAlign = 256;

inline size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

// What the sort may ask for on top of the arrays, for n rows of 4 + 4 bytes:
// a second copy of keys and values (8 n), the onesweep look-back states (256
// words per block of at least 256 rows: 4 n), histograms and alignment.
inline size_t sort_tmp_bound(uint32_t n) { return (size_t)16 * n + (64u << 10); }

inline unsigned key_bits(uint32_t n_keys) {  // ceil(log2(n_keys + 1)): n_keys itself is a key
  unsigned b = 1;
  while (b < 32 && (n_keys >> b)) ++b;
  return b;
}

hipError_t sort_pairs(void* tmp, size_t& tmp_bytes, const KeyOrder& ko, uint32_t n, uint32_t n_keys, hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, ko.keys_in, ko.keys, ko.slots_in, ko.slots, (size_t)n, 0u,
                                   key_bits(n_keys), s);
}

__global__ __launch_bounds__(kThreads) void heads_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                         uint32_t n_keys, uint32_t* __restrict__ heads,
                                                         uint32_t* __restrict__ n_heads) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= n) return;
  const uint32_t k = keys[p];
  if (k < n_keys && (p == 0 || keys[p - 1] != k)) heads[atomicAdd(n_heads, 1u)] = p;  // at most n of them
}

}  // namespace

size_t keyorder_work_bytes(uint32_t n) {
  // keys_in, slots_in, keys, slots, heads | n_heads | base | the sort's
  return 5 * align_up((size_t)4 * n) + kAlign + align_up((size_t)8 * n) + align_up(sort_tmp_bound(n));
}

bool keyorder_carve(void* d_work, size_t work_bytes, uint32_t n, KeyOrder* ko) {
  const size_t a4 = align_up((size_t)4 * n), fixed = 5 * a4 + kAlign + align_up((size_t)8 * n);
  if (work_bytes < fixed) return false;
  uint8_t* p = (uint8_t*)d_work;
  ko->keys_in = (uint32_t*)p;
  ko->slots_in = (uint32_t*)(p + a4);
  ko->keys = (uint32_t*)(p + 2 * a4);
  ko->slots = (uint32_t*)(p + 3 * a4);
  ko->heads = (uint32_t*)(p + 4 * a4);
  ko->n_heads = (uint32_t*)(p + 5 * a4);
  ko->base = (uint64_t*)(p + 5 * a4 + kAlign);
  ko->sort_tmp = p + fixed;
  ko->sort_tmp_bytes = work_bytes - fixed;
  return true;
}

hipError_t keyorder_check(const KeyOrder& ko, uint32_t n, uint32_t n_keys, hipStream_t s, bool* fits) {
  size_t need = 0;
  const hipError_t e = sort_pairs(nullptr, need, ko, n, n_keys, s);  // a size query: nothing is launched
  *fits = e == hipSuccess && need <= ko.sort_tmp_bytes;
  return e;
}

hipError_t keyorder_sort(const KeyOrder& ko, uint32_t n, uint32_t n_keys, hipStream_t s) {
  hipError_t e = hipMemsetAsync(ko.n_heads, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  size_t bytes = ko.sort_tmp_bytes;
  e = sort_pairs(ko.sort_tmp, bytes, ko, n, n_keys, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(heads_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, ko.keys, n, n_keys,
                     ko.heads, ko.n_heads);
  return hipGetLastError();
}

}  // namespace wgcs
