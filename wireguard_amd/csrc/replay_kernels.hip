// replay_kernels.hip -- the two per-keypair steps of the packet path on
// device-resident batches (include/wgcsum.h):
//   replay    keypair.replayFilter.Validate              device/receive.go:414-420, replay/replay.go
//   assign    keypair.sendNonce.Add(1) and its limit     device/send.go:383-390
// Both are sequential per key, and both use the wave walk of wgcs_keyorder.h:
// every row of a trip is decided from the state before the trip, so the wave
// never walks a segment row by row.
//
// The trip rule of the replay filter, for rows v_0 .. v_{m-1} of one key on the
// state (L, ring), with ok_i = v_i < limit:
//   M_i   = max(L, max{v_j : j < i, ok_j})         what `last` is when row i's turn comes
//   win_i = ok_i && (v_i > M_i || M_i - v_i <= 8128)
//   dup_i = some j < i with ok_j and v_j == v_i     an earlier row of the trip set the bit
//   old_i = win_i && block(v_i) <= block(L) && the bit of v_i is set in ring
//   row i is accepted iff win_i && !dup_i && !old_i
//   L'    = max(L, max{v_j : ok_j});  blocks block(L)+1 .. block(L)+min(block(L')-block(L), 128)
//           are cleared, then the bit of every win_i row with block(L')-block(v_i) < 128 is set.
// Why old_i may read the ring as it was before the trip: a win_i row is at
// most 127 blocks behind M_i, and the blocks cleared before its turn are
// block(L)+1 .. block(M_i), which meet block(v_i) mod 128 only from 128 blocks
// on; so a block at or below block(L) is untouched but for the bits that
// earlier rows of the trip set (dup_i), and a block above block(L) was cleared
// on the way.  On every state that Validate can reach, block(v_i) <= block(L)
// with a set bit is the same as v_i <= L with a set bit.  tests/replay_ref.py
// holds this rule as plain Python and tests/test_replay_ref.py checks it, state
// for state, against the sequential filter.
//
// A wave keeps its filter in LDS for the whole segment (1 KiB; only the wave
// itself touches it, so wave-level ordering is all it needs).  Reading a row's
// bit is one LDS read, the clear is a store by the lanes that own the stale
// words, and the rows set their bits with LDS atomic ORs.  The value an OR
// returns tells whether the bit was already there: for a row that is not
// old_i that can only be an equal value of the same trip, whichever lane got
// there first.  Only then -- or when a win_i row lies 128 blocks or more
// behind L', so that nobody sets its bit -- does the wave run the 64-step
// loop that finds dup_i by lane order; a trip without such a collision costs
// the scan and five LDS operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_replay.h"
#include "wgcs_route_walk.h"

namespace wgcs {

namespace {

constexpr int kThreads = kKeyOrderThreads, kWavesPerBlock = kKeyOrderWaves;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

__device__ inline uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ---------------------------------------------------------------------- replay
// verdict may alias pkt_len: row i is read, then written, by the lane that owns it
__global__ __launch_bounds__(kThreads) void replay_keys_kernel(const wgcs_aead_pkt* __restrict__ pkts,
                                                               const int32_t* pkt_len, uint32_t n, uint32_t n_keys,
                                                               int32_t* verdict, uint32_t* __restrict__ keys_in,
                                                               uint32_t* __restrict__ slots_in) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t len = pkt_len[i];
  const uint32_t key = pkts[i].key;
  // every message that Open decrypted consumes its counter: receive.go:414-420 precedes the trim
  const bool takes = key < n_keys && (len >= 0 || len == WGCS_ERR_PACKET_TOO_SHORT);
  verdict[i] = len;
  keyorder_put(keys_in, slots_in, i, takes ? key : n_keys);
}

__global__ __launch_bounds__(kThreads) void replay_groups_kernel(const uint32_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ slots,
                                                                 const uint32_t* __restrict__ heads,
                                                                 const uint32_t* __restrict__ n_heads, uint32_t n,
                                                                 const uint64_t* __restrict__ counter, uint64_t limit,
                                                                 wgcs_replay_filter* __restrict__ filters,
                                                                 int32_t* __restrict__ verdict) {
  __shared__ unsigned long long lds_ring[kWavesPerBlock][kReplayBlocks];
  unsigned long long* const ring = lds_ring[threadIdx.x / kWave];
  const int lane = threadIdx.x & (kWave - 1);
  for (KeySegments seg(keys, heads, n_heads, n); seg.next();) {
    wgcs_replay_filter* const f = filters + seg.key;
    uint64_t L = f->last;
    wave_sync();  // the segment before this one has read its ring out
    ring[lane] = f->ring[lane];
    ring[lane + kWave] = f->ring[lane + kWave];
    wave_sync();
    seg.trips(lane, [&](bool mine, uint64_t pos, int m) {
      const uint32_t slot = mine ? slots[pos] : 0;
      const uint64_t v = mine ? counter[slot] : 0;
      const bool ok = mine && v < limit;
      // M_i: an inclusive max scan over the rows that may move `last`, shifted by one lane
      const uint64_t inc = wave_scan(ok ? v : 0, lane, WaveMax());
      uint64_t exc = __shfl_up(inc, 1);
      if (lane == 0) exc = 0;
      const uint64_t M = max64(L, exc);
      const uint64_t Lnew = max64(L, readlane64(inc, kWave - 1));
      const bool win = ok && (v > M || M - v <= kReplayWindow);
      // old_i: the row's bit in the ring as the trip found it
      const uint32_t b = (uint32_t)(v >> kReplayBlockShift) & (uint32_t)kReplayBlockMask;
      const unsigned long long bit = 1ull << (v & kReplayBitMask);
      const bool old = win && (v >> kReplayBlockShift) <= (L >> kReplayBlockShift) && (ring[b] & bit);
      wave_sync();
      // the window moves: blocks block(L)+1 .. block(L)+adv go stale
      uint64_t adv = (Lnew >> kReplayBlockShift) - (L >> kReplayBlockShift);
      if (adv > kReplayBlocks) adv = kReplayBlocks;
      const uint64_t first = (L >> kReplayBlockShift) + 1;
      if ((((uint64_t)lane - first) & kReplayBlockMask) < adv) ring[lane] = 0;
      if ((((uint64_t)(lane + kWave) - first) & kReplayBlockMask) < adv) ring[lane + kWave] = 0;
      wave_sync();
      const bool setf = win && (Lnew >> kReplayBlockShift) - (v >> kReplayBlockShift) < kReplayBlocks;
      const bool hit = setf && (atomicOr(&ring[b], bit) & bit) && !old;  // an equal value of this trip
      wave_sync();
      bool dup = false;
      if (__ballot(hit || (win && !setf)) != 0) {  // wave-uniform
        const int flags = ok ? 1 : 0;
        for (int j = 0; j < m; ++j) {  // row j of the trip, as scalars
          const uint64_t vj = readlane64(v, j);
          const int fj = __builtin_amdgcn_readlane(flags, j);
          if (fj && j < lane && vj == v) dup = true;
        }
      }
      if (mine && !(win && !dup && !old)) verdict[slot] = WGCS_ERR_REPLAY;
      L = Lnew;
    });
    if (lane == 0) f->last = L;
    wave_sync();
    f->ring[lane] = ring[lane];
    f->ring[lane + kWave] = ring[lane + kWave];
  }
}

// ---------------------------------------------------------------------- assign
__global__ __launch_bounds__(kThreads) void assign_keys_kernel(
    const int32_t* __restrict__ count, const int32_t* __restrict__ status, const uint32_t* __restrict__ peer,
    uint32_t n_jobs, uint32_t max_segs, const wgcs_session_slot* __restrict__ peer_keys, uint32_t n_slots,
    uint32_t n_keys, uint32_t* __restrict__ keys_in, uint32_t* __restrict__ slots_in, int32_t* __restrict__ nbufs,
    uint32_t* __restrict__ job_key, uint64_t* __restrict__ base) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_jobs) return;
  const int32_t c = count[j];
  uint32_t key = n_keys;
  if (status[j] == 0 && c >= 1 && (uint32_t)c <= max_segs) {
    // one super-packet has one destination: the first slot's peer is the job's
    const uint32_t p = peer[(uint64_t)j * max_segs];
    if (p != WGCS_PEER_NONE) {
      const uint32_t k = session_get(peer_keys, n_slots, p);
      if (k < n_keys) key = k;
    }
  }
  keyorder_put(keys_in, slots_in, j, key);
  nbufs[j] = 0;  // dropped, until the key's wave keeps it
  job_key[j] = kNoKey;
  base[j] = 0;
}

__global__ __launch_bounds__(kThreads) void assign_groups_kernel(const uint32_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ slots,
                                                                 const uint32_t* __restrict__ heads,
                                                                 const uint32_t* __restrict__ n_heads, uint32_t n_jobs,
                                                                 const int32_t* __restrict__ count, uint64_t limit,
                                                                 uint64_t* __restrict__ send_nonce,
                                                                 int32_t* __restrict__ nbufs,
                                                                 uint32_t* __restrict__ job_key,
                                                                 uint64_t* __restrict__ base) {
  const int lane = threadIdx.x & (kWave - 1);
  for (KeySegments seg(keys, heads, n_heads, n_jobs); seg.next();) {
    const uint32_t key = seg.key;
    uint64_t cur = send_nonce[key];
    bool dead = false;  // a job of this key did not fit: send.go:386
    seg.trips(lane, [&](bool mine, uint64_t pos, int m) {
      const uint32_t j = mine ? slots[pos] : 0;
      const uint64_t c = mine ? (uint64_t)count[j] : 0;  // 1 .. max_segs: assign_keys_kernel checked
      const uint64_t inc = wave_scan(c, lane, WaveSum());  // at most 2^24 jobs of < 2^32 each: no wrap
      // job j takes [cur + inc - c, cur + inc): it fits iff cur + inc <= limit, without forming the sum
      const uint64_t room = limit > cur ? limit - cur : 0;
      const bool fit = mine && !dead && inc <= room;
      const uint64_t nofit = __ballot(mine && !fit);
      const int first = nofit ? __ffsll((unsigned long long)nofit) - 1 : kWave;
      if (mine && lane < first) {
        nbufs[j] = (int32_t)c;
        job_key[j] = key;
        base[j] = cur + (inc - c);
      }
      if (nofit) dead = true;
      else cur += readlane64(inc, m - 1);
    });
    if (lane == 0) send_nonce[key] = dead ? limit : cur;
  }
}

__global__ __launch_bounds__(kThreads) void assign_rows_kernel(const int32_t* __restrict__ sizes,
                                                               const int32_t* __restrict__ nbufs,
                                                               const uint32_t* __restrict__ job_key,
                                                               const uint64_t* __restrict__ base, uint32_t n_rows,
                                                               uint32_t max_segs, uint64_t stride,
                                                               wgcs_aead_pkt* __restrict__ pkts) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n_rows) return;
  const uint32_t j = q / max_segs, k = q - j * max_segs;
  wgcs_aead_pkt pk;
  pk.off = (uint64_t)q * stride;
  if ((int32_t)k < nbufs[j]) {
    pk.counter = base[j] + k;
    pk.len = (uint32_t)sizes[q];
    pk.key = job_key[j];
  } else {  // a row that carries nothing names no key: seal refuses it untouched
    pk.counter = 0;
    pk.len = 0;
    pk.key = kNoKey;
  }
  pkts[q] = pk;
}

}  // namespace

hipError_t launch_replay(const KeyOrder& ko, const wgcs_aead_pkt* pkts, const int32_t* pkt_len,
                         const uint64_t* counter, uint32_t n, wgcs_replay_filter* filters, uint32_t n_keys,
                         uint64_t limit, int32_t* verdict, hipStream_t s) {
  hipLaunchKernelGGL(replay_keys_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, pkts, pkt_len, n, n_keys, verdict,
                     ko.keys_in, ko.slots_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n, n_keys, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(replay_groups_kernel, dim3(keyorder_group_blocks(n)), dim3(kThreads), 0, s, ko.keys, ko.slots, ko.heads,
                     ko.n_heads, n, counter, limit, filters, verdict);
  return hipGetLastError();
}

hipError_t launch_send_assign(const KeyOrder& ko, const int32_t* sizes, const uint32_t* peer, const int32_t* count,
                              const int32_t* status, uint32_t n_jobs, uint32_t max_segs, uint64_t stride,
                              const wgcs_session_slot* peer_keys, uint32_t n_slots, uint64_t* send_nonce,
                              uint32_t n_keys, uint64_t limit, wgcs_aead_pkt* pkts, int32_t* nbufs, uint32_t* job_key,
                              hipStream_t s) {
  hipLaunchKernelGGL(assign_keys_kernel, dim3(keyorder_blocks(n_jobs)), dim3(kThreads), 0, s, count, status, peer, n_jobs,
                     max_segs, peer_keys, n_slots, n_keys, ko.keys_in, ko.slots_in, nbufs, job_key, ko.base);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n_jobs, n_keys, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(assign_groups_kernel, dim3(keyorder_group_blocks(n_jobs)), dim3(kThreads), 0, s, ko.keys, ko.slots,
                     ko.heads, ko.n_heads, n_jobs, count, limit, send_nonce, nbufs, job_key, ko.base);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(assign_rows_kernel, dim3(keyorder_blocks(n_jobs * max_segs)), dim3(kThreads), 0, s, sizes, nbufs,
                     job_key, ko.base, n_jobs * max_segs, max_segs, stride, pkts);
  return hipGetLastError();
}

}  // namespace wgcs
