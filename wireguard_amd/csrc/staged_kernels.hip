// staged_kernels.hip -- the staged queue (peer.qus.staged) on device-resident rings
// (include/wgcsum.h), the row functions of wgcs_staged.h:
//   stage     StagePackets and the re-staging of send.go:402-407         send.go:331-350
//     staged_keys_kernel      one lane per slot: d_where's default, and per job its peer row as the
//                             key, its packets, and the call's count of staged jobs
//     (the key order of wgcs_keyorder.h over the peer rows)
//     staged_groups_kernel    the wave walk, twice per peer: the packets of its jobs summed, the
//                             ring words written by one lane, then every job's place in the ring
//     staged_copy_kernel      16 lanes per slot: the scatter copy into the rings
//   release   SendStagedPackets up to the nonce loop                     send.go:363-426
//     staged_release_verdict_kernel / _commit_kernel   the weighted form of wgcs_compact.h over the
//                             peer rows: a ready row weighs its packets
//     staged_release_copy_kernel   a block per released ring: the gather copy into the job table,
//                             the tail rows, and the ring words put back to empty
//   flush     FlushStagedPackets, one lane per peer row                  send.go:352-361
// On most send batches nothing is refused: the keys kernel counts the staged jobs into the
// workspace, and the groups and copy kernels return on a zero count, so the call then costs its
// launches and the sort of n_jobs equal keys.  Launch shapes do not depend on device data.
//
// The copies move whole 16-byte rows of [16, 16 + size) -- both ends are 16-byte aligned by the
// layout -- 16 lanes a packet, four rows a lane in flight (1 KiB per packet and trip), and the
// last size % 16 bytes one byte a lane, so no byte past 16 + size of a slot is written.  Every
// ring slot and every output job has one writer, and the ring words of a peer one lane: which
// wave runs first changes no byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_compact.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_staged.h"

namespace wgcs {

namespace {

constexpr int kThreads = kCompactThreads;
static_assert(kThreads == kKeyOrderThreads, "one block shape for the compacting and the key-order kernels");
constexpr int kGroup = 16;                             // the lanes that share a packet
constexpr int kGroupsPerBlock = kThreads / kGroup;
constexpr int kRowsInFlight = 4;                       // 16-byte rows a lane loads before it stores any
constexpr uint32_t kMaxRingBlocks = 4096;              // the release copy strides over the rings

// dst[0, size) = src[0, size) by the 16 lanes of a group, l the lane's place in it; both 16-byte aligned
__device__ inline void copy_packet(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t size,
                                   uint32_t l) {
  const uint32_t rows = size >> 4;
  const uint4* const s4 = reinterpret_cast<const uint4*>(src);
  uint4* const d4 = reinterpret_cast<uint4*>(dst);
  for (uint32_t r0 = 0; r0 < rows; r0 += kGroup * kRowsInFlight) {
    uint4 v[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const uint32_t r = r0 + l + kGroup * u;
      v[u] = r < rows ? s4[r] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const uint32_t r = r0 + l + kGroup * u;
      if (r < rows) d4[r] = v[u];
    }
  }
  if (l < (size & 15u)) dst[16 * rows + l] = src[16 * rows + l];
}

// ----------------------------------------------------------------------- stage
__global__ __launch_bounds__(kThreads) void staged_keys_kernel(
    const int32_t* __restrict__ sizes, const uint32_t* __restrict__ peer, const int32_t* __restrict__ count,
    const int32_t* __restrict__ status_in, const int32_t* __restrict__ status_out,
    const uint32_t* __restrict__ job_key, uint32_t n_rows, uint32_t max_segs, uint64_t stride,
    const uint32_t* __restrict__ peer_rows, uint32_t n_ids, uint32_t n_peers, uint32_t* __restrict__ keys_in,
    uint32_t* __restrict__ slots_in, uint64_t* __restrict__ place, uint32_t* n_stage, uint32_t* __restrict__ where) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  bool staged = false;
  if (q < n_rows) {
    where[q] = WGCS_STAGED_NONE;
    const uint32_t j = q / max_segs;
    if (q == j * max_segs) {  // the job's first slot speaks for the job
      const uint32_t row =
          staged_job_row(j, peer, count, status_in, status_out, job_key, max_segs, peer_rows, n_ids, n_peers);
      const uint32_t nv = row != WGCS_PEER_NONE ? staged_segs_ok(j, (uint32_t)count[j], sizes, max_segs, stride) : 0;
      staged = nv != 0;
      keyorder_put(keys_in, slots_in, j, staged ? row : n_peers);
      place[j] = nv;  // until the peer's wave turns it into the job's place
    }
  }
  const int c = __syncthreads_count(staged);
  if (threadIdx.x == 0 && c) atomicAdd(n_stage, (uint32_t)c);
}

__global__ __launch_bounds__(kThreads) void staged_groups_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ heads,
    const uint32_t* __restrict__ n_heads, const uint32_t* __restrict__ n_stage, uint32_t n_jobs, uint32_t cap,
    uint32_t* len, uint32_t* head, uint32_t* lost, uint64_t* place) {
  if (*n_stage == 0) return;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  for (KeySegments seg(keys, heads, n_heads, n_jobs); seg.next();) {
    const uint32_t r = seg.key;
    uint32_t m = 0;  // the packets of the peer's jobs, 64 jobs a trip
    seg.trips(lane, [&](bool mine, uint64_t pos, int) {
      const uint32_t nv = mine ? (uint32_t)place[slots[pos]] : 0;
      m += (uint32_t)__builtin_amdgcn_readlane((int)wave_scan(nv, lane, WaveSum()), kWave - 1);
    });
    const StagedGroup g = staged_group(len[r], head[r], m, cap);
    uint32_t k0 = 0;  // the rank of the trip's first packet
    seg.trips(lane, [&](bool mine, uint64_t pos, int) {
      const uint32_t j = mine ? slots[pos] : 0;
      const uint32_t nv = mine ? (uint32_t)place[j] : 0;
      const uint32_t inc = wave_scan(nv, lane, WaveSum());
      if (mine) place[j] = staged_place(g, k0 + inc - nv, nv, cap);
      k0 += (uint32_t)__builtin_amdgcn_readlane((int)inc, kWave - 1);
    });
    if (lane == 0) {
      head[r] = g.head;
      len[r] = g.len;
      lost[r] += g.evicted;
    }
  }
}

__global__ __launch_bounds__(kThreads) void staged_copy_kernel(
    const uint8_t* __restrict__ arena, const int32_t* __restrict__ sizes, const int32_t* __restrict__ count,
    uint32_t n_rows, uint32_t max_segs, uint64_t stride, const uint32_t* __restrict__ keys_in,
    const uint64_t* __restrict__ place, const uint32_t* __restrict__ n_stage, uint32_t n_peers, uint32_t cap,
    int32_t* __restrict__ slot_size, uint8_t* __restrict__ ring, uint32_t* __restrict__ where) {
  if (*n_stage == 0) return;
  const uint32_t q = blockIdx.x * kGroupsPerBlock + threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  if (q >= n_rows) return;
  const uint32_t j = q / max_segs;
  const uint32_t r = keys_in[j];
  if (r >= n_peers) return;  // not staged: d_where holds its default
  const uint32_t w = staged_seg_where(j, q - j * max_segs, sizes, count, max_segs, stride, r, place[j], cap);
  if (w == WGCS_STAGED_NONE) return;
  if (l == 0) where[q] = w;
  if (w == WGCS_STAGED_EVICTED) return;
  const int32_t size = sizes[q];
  if (l == 0) slot_size[w] = size;
  copy_packet(arena + (uint64_t)q * stride + kStagedHead, ring + (uint64_t)w * stride + kStagedHead, (uint32_t)size, l);
}

// --------------------------------------------------------------------- release
// block_weight[b] = the packets of block b's candidates
__global__ __launch_bounds__(kThreads) void staged_release_verdict_kernel(
    int64_t now, const uint32_t* __restrict__ len, const wgcs_keypairs* __restrict__ kp,
    const uint64_t* __restrict__ send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey, uint32_t n_peers,
    int32_t* __restrict__ status, uint32_t* __restrict__ block_weight) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  uint32_t w = 0;
  if (r < n_peers) {
    const int32_t v = status[r] = staged_release_verdict(r, now, len, kp, send_nonce, n_keys, limit, rekey);
    if (v == WGCS_STAGED_RELEASED) w = len[r];
  }
  compact_weigh_block(w, block_weight);
}

__global__ __launch_bounds__(kThreads) void staged_release_commit_kernel(
    const uint32_t* __restrict__ len, uint32_t n_peers, uint32_t n_out_max, const uint32_t* __restrict__ weight_below,
    uint32_t* __restrict__ base, uint32_t* n_out, int32_t* __restrict__ status) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  const bool cand = r < n_peers && status[r] == WGCS_STAGED_RELEASED;
  const uint32_t w = cand ? len[r] : 0;  // not 0: the verdict saw a queue
  const uint32_t P = compact_weighted_rank(w, weight_below);
  if (cand) status[r] = staged_release_commit(r, P, w, n_out_max, base, n_out);
  else if (r < n_peers) base[r] = kStagedNoBase;
}

__global__ __launch_bounds__(kThreads) void staged_release_copy_kernel(
    const wgcs_peer_key* __restrict__ table, uint32_t* len, uint32_t* head, const int32_t* __restrict__ slot_size,
    const uint8_t* __restrict__ ring, uint32_t n_peers, uint32_t cap, uint64_t stride,
    const uint32_t* __restrict__ base, uint32_t n_out_max, uint8_t* __restrict__ out, uint32_t* __restrict__ out_peer,
    int32_t* __restrict__ out_count, int32_t* __restrict__ out_sizes, int32_t* __restrict__ out_status,
    const uint32_t* __restrict__ n_out) {
  const uint32_t n = *n_out;  // final: the commit kernel is done
  for (uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x; k < n_out_max; k += (uint64_t)gridDim.x * kThreads)
    if (k >= n) staged_out_tail((uint32_t)k, out_peer, out_count, out_sizes, out_status);
  const uint32_t g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  for (uint32_t r = blockIdx.x; r < n_peers; r += gridDim.x) {
    const uint32_t P = base[r];
    if (P == kStagedNoBase) continue;  // the same for the whole block
    const uint32_t L = len[r], h = head[r], peer = table[r].peer;
    for (uint32_t i = g; i < L; i += kGroupsPerBlock) {
      const uint32_t slot = r * cap + ((h + i) & (cap - 1)), k = P + i;
      const int32_t size = staged_slot_size(slot_size[slot], stride);
      if (l == 0) staged_out_row(k, peer, size, out_peer, out_count, out_sizes, out_status);
      copy_packet(ring + (uint64_t)slot * stride + kStagedHead, out + (uint64_t)k * stride + kStagedHead, (uint32_t)size,
                  l);
    }
    __syncthreads();  // every group has read the row's words
    if (threadIdx.x == 0) {
      len[r] = 0;
      head[r] = 0;
    }
  }
}

// ----------------------------------------------------------------------- flush
__global__ __launch_bounds__(kThreads) void staged_flush_kernel(const uint32_t* __restrict__ actions, uint32_t* len,
                                                                uint32_t* head, uint32_t* lost, uint32_t n_peers) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r < n_peers) staged_flush_row(r, actions, len, head, lost);
}

}  // namespace

hipError_t launch_staged_stage(const KeyOrder& ko, const uint8_t* arena, const int32_t* sizes, const uint32_t* peer,
                               const int32_t* count, const int32_t* status_in, const int32_t* status_out,
                               const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, const uint32_t* peer_rows,
                               uint32_t n_ids, const StagedRings& st, uint32_t* where, hipStream_t s) {
  const uint32_t n_rows = n_jobs * max_segs;
  uint32_t* const n_stage = ko.n_heads + 1;  // the second word of the 256 bytes that hold *n_heads
  hipError_t e = hipMemsetAsync(n_stage, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(staged_keys_kernel, dim3(compact_blocks(n_rows)), dim3(kThreads), 0, s, sizes, peer, count,
                     status_in, status_out, job_key, n_rows, max_segs, st.stride, peer_rows, n_ids, st.n_peers,
                     ko.keys_in, ko.slots_in, ko.base, n_stage, where);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n_jobs, st.n_peers, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(staged_groups_kernel, dim3(keyorder_group_blocks(n_jobs)), dim3(kThreads), 0, s, ko.keys, ko.slots, ko.heads,
                     ko.n_heads, n_stage, n_jobs, st.cap, st.len, st.head, st.lost, ko.base);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(staged_copy_kernel, dim3((n_rows + kGroupsPerBlock - 1) / kGroupsPerBlock), dim3(kThreads), 0, s,
                     arena, sizes, count, n_rows, max_segs, st.stride, ko.keys_in, ko.base, n_stage, st.n_peers, st.cap,
                     st.slot_size, st.ring, where);
  return hipGetLastError();
}

hipError_t launch_staged_release(int64_t now, const wgcs_peer_key* table, const wgcs_keypairs* kp,
                                 const uint64_t* send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey,
                                 const StagedRings& st, uint32_t n_out_max, uint8_t* out, uint32_t* out_peer,
                                 int32_t* out_count, int32_t* out_sizes, int32_t* out_status, uint32_t* n_out,
                                 int32_t* status, uint32_t* work, hipStream_t s) {
  const uint32_t n_blocks = compact_blocks(st.n_peers);
  uint32_t* const block_weight = work;
  uint32_t* const base = work + ((n_blocks + 63u) & ~63u);  // one word per peer row behind the block words
  hipError_t e;
  if (n_blocks) {
    hipLaunchKernelGGL(staged_release_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, st.len, kp, send_nonce,
                       n_keys, limit, rekey, st.n_peers, status, block_weight);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = launch_compact_scan(block_weight, n_blocks, n_out_max, n_out, s)) != hipSuccess) return e;
  if (n_blocks) {
    hipLaunchKernelGGL(staged_release_commit_kernel, dim3(n_blocks), dim3(kThreads), 0, s, st.len, st.n_peers, n_out_max,
                       block_weight, base, n_out, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const uint32_t tail_blocks = compact_blocks(n_out_max);
  uint32_t blocks = st.n_peers > tail_blocks ? st.n_peers : tail_blocks;  // a block a ring, and the tail rows
  if (blocks == 0) return hipSuccess;
  if (blocks > kMaxRingBlocks) blocks = kMaxRingBlocks;
  hipLaunchKernelGGL(staged_release_copy_kernel, dim3(blocks), dim3(kThreads), 0, s, table, st.len, st.head,
                     st.slot_size, st.ring, st.n_peers, st.cap, st.stride, base, n_out_max, out, out_peer, out_count,
                     out_sizes, out_status, n_out);
  return hipGetLastError();
}

hipError_t launch_staged_flush(const uint32_t* actions, uint32_t* len, uint32_t* head, uint32_t* lost, uint32_t n_peers,
                               hipStream_t s) {
  hipLaunchKernelGGL(staged_flush_kernel, dim3(compact_blocks(n_peers)), dim3(kThreads), 0, s, actions, len, head, lost,
                     n_peers);
  return hipGetLastError();
}

}  // namespace wgcs
