// write_kernels.hip -- gfx950: the Write calls of every receive batch, one per
// peer, built where the verdicts are (include/wgcsum.h, wgcs_write_build_batch).
// The rule is wgcs_write_plan.h's write_plan_batch; this is its wave form, and
// the row predicates and row images are that header's own functions.
//
// One 64-lane wave owns one batch of at most 128 rows: lane l holds rows l and
// l + 64 in registers.  Four batches per workgroup; nothing is shared between
// waves, no LDS, no atomics, and all control flow is wave-uniform.
//
// Group discovery makes one trip per group: ballot the validated rows that no
// group has taken yet, broadcast the peer of the lowest one, ballot the rows of
// that peer.  A kept row's place among its call's buffers is its rank in the
// ballot of the group's kept rows (mbcnt), behind the kept rows of the groups
// before it.  Group g's call and accounting rows wait in the registers of lane
// g & 63 until the loop is over: only then is it known whether the batch is
// refused, and a refused batch leaves nothing half-built.  So every row of
// every output is stored exactly once, by one lane.  Past calls_per_batch a
// trip only counts, so that d_n_groups is right for a refused batch too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_write_plan.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256, kWave = 64, kWavesPerBlock = kThreads / kWave;
// rx_bytes of a group of up to this many rows is summed by reading its lanes one by one; a larger
// group takes the wave reduction.  Measured: batches of one-row groups gain a
// fifth of the launch over the reduction; for eight-row groups the reduction was the faster by
// a few per cent
constexpr uint32_t kScalarSum = 4;

struct GroupRegs {  // one group's call and accounting rows, in the lane that will store them
  uint32_t peer;
  int32_t tail;
  uint32_t flags, n_valid;
  uint64_t rx_bytes;
  uint32_t first, n;
};

__device__ inline uint32_t lanes_below(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

__device__ inline uint64_t wave_sum64(uint64_t x) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d);
  return x;
}

// d_bufs and d_calls are 16-byte aligned tables of 16-byte rows: one store each
template <typename Row>
__device__ inline void store16(Row* dst, const Row& r) {
  static_assert(sizeof(Row) == 16, "a 16-byte row");
  uint4 v;
  __builtin_memcpy(&v, &r, 16);
  *reinterpret_cast<uint4*>(dst) = v;
}

__global__ __launch_bounds__(kThreads) void write_build_kernel(
    const wgcs_aead_pkt* __restrict__ pkts, const int32_t* __restrict__ verdict, uint32_t n_msgs, uint32_t n_batches,
    const uint32_t* __restrict__ key_peer, uint32_t n_keys, int32_t offset, uint32_t cap, uint32_t gro_flags,
    uint32_t calls_per_batch, wgcs_gro_buf* __restrict__ bufs, wgcs_gro_call* __restrict__ calls,
    wgcs_write_group* __restrict__ groups, int32_t* __restrict__ n_groups, int32_t* __restrict__ status) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t b = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave);
  if (b >= n_batches) return;  // wave-uniform: the last workgroup's spare waves
  const uint32_t q0 = b * n_msgs;  // n_batches * n_msgs <= 2^28

  // ---- the batch's rows: lane l has rows l and l + 64
  uint64_t off[2];
  uint32_t len[2], peer[2], dest[2] = {0, 0};
  int32_t vd[2];
  bool kept[2], bad = false;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t i = lane + kWave * h;
    off[h] = 0, len[h] = 0, vd[h] = 0, peer[h] = WGCS_PEER_NONE;
    if (i < n_msgs) {
      const wgcs_aead_pkt* p = pkts + q0 + i;
      off[h] = p->off;
      len[h] = p->len;
      vd[h] = verdict[q0 + i];
      peer[h] = write_row_peer(p->key, vd[h], key_peer, n_keys);
    }
    kept[h] = write_row_kept(peer[h], vd[h]);
    bad = bad || (kept[h] && !write_row_fits(offset, vd[h], cap));
  }
  const bool fits = __ballot(bad) == 0;

  // ---- one trip per group
  uint64_t un0 = __ballot(peer[0] != WGCS_PEER_NONE), un1 = __ballot(peer[1] != WGCS_PEER_NONE);
  uint32_t ng = 0, kept_total = 0;
  GroupRegs lo = {WGCS_PEER_NONE, -1, 0, 0, 0, q0, 0}, hi = lo;  // groups lane and lane + 64
  while (un0 | un1) {
    const int src = __builtin_amdgcn_readfirstlane(un0 ? __builtin_ctzll(un0) : __builtin_ctzll(un1));
    const uint32_t P = (uint32_t)(un0 ? __builtin_amdgcn_readlane((int)peer[0], src)
                                      : __builtin_amdgcn_readlane((int)peer[1], src));
    const bool in0 = peer[0] == P, in1 = peer[1] == P;  // P is a peer: rows that take no part never match
    const uint64_t m0 = __ballot(in0), m1 = __ballot(in1);
    un0 &= ~m0;
    un1 &= ~m1;
    if (ng < calls_per_batch) {
      const uint64_t k0 = __ballot(in0 && kept[0]), k1 = __ballot(in1 && kept[1]);
      const uint32_t n0 = (uint32_t)__popcll(k0), n = n0 + (uint32_t)__popcll(k1);
      const uint32_t first = q0 + kept_total;
      if (in0 && kept[0]) dest[0] = first + lanes_below(k0);
      if (in1 && kept[1]) dest[1] = first + n0 + lanes_below(k1);
      GroupRegs g;
      g.peer = P;
      g.tail = (int32_t)(q0 + (m1 ? 2 * kWave - 1 - __builtin_clzll(m1) : kWave - 1 - __builtin_clzll(m0)));
      g.flags = __ballot((in0 && write_row_data(len[0])) || (in1 && write_row_data(len[1]))) ? WGCS_GROUP_DATA : 0u;
      g.n_valid = (uint32_t)(__popcll(m0) + __popcll(m1));
      if (g.n_valid <= kScalarSum) {  // wave-uniform: a small group's lengths, row by row on the scalar unit
        g.rx_bytes = 0;
        for (uint64_t m = m0; m; m &= m - 1)
          g.rx_bytes += (uint32_t)__builtin_amdgcn_readlane((int)len[0], __builtin_ctzll(m));
        for (uint64_t m = m1; m; m &= m - 1)
          g.rx_bytes += (uint32_t)__builtin_amdgcn_readlane((int)len[1], __builtin_ctzll(m));
      } else {
        g.rx_bytes = wave_sum64((uint64_t)(in0 ? len[0] : 0u) + (uint64_t)(in1 ? len[1] : 0u));
      }
      g.first = first;
      g.n = n;
      if (lane == (ng & (kWave - 1))) {
        if (ng < (uint32_t)kWave) lo = g;
        else hi = g;
      }
      kept_total += n;
    }
    ++ng;
  }

  // ---- every row of every output, once
  const int32_t st = !fits ? WGCS_ERR_OUT_OF_RANGE : ng > calls_per_batch ? WGCS_ERR_BATCH_FULL : WGCS_OK;
  const bool ok = st == WGCS_OK;
  const uint32_t used = ok ? ng : 0, total = ok ? kept_total : 0;  // total <= n_msgs: each kept row counts once
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t i = lane + kWave * h;
    if (ok && kept[h]) store16(bufs + dest[h], write_buf_row(off[h], offset, vd[h], cap));  // dest < q0 + total
    if (i >= total && i < n_msgs) store16(bufs + q0 + i, write_buf_zero());
    if (i < calls_per_batch) {  // calls_per_batch <= n_msgs <= 128
      const GroupRegs& g = h ? hi : lo;
      const uint32_t c = b * calls_per_batch + i;
      wgcs_write_group w = write_group_unused();
      if (i < used) {
        w.peer = g.peer;
        w.tail = g.tail;
        w.flags = g.flags;
        w.n_valid = g.n_valid;
        w.rx_bytes = g.rx_bytes;
      }
      store16(calls + c, i < used ? write_call_row(g.first, g.n, offset, gro_flags)
                                  : write_call_row(q0, 0, offset, gro_flags));
      groups[c] = w;
    }
  }
  if (lane == 0) {
    n_groups[b] = (int32_t)ng;
    status[b] = st;
  }
}

}  // namespace

hipError_t launch_write_build(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n_msgs, uint32_t n_batches,
                              const uint32_t* key_peer, uint32_t n_keys, int32_t offset, uint32_t cap,
                              uint32_t gro_flags, uint32_t calls_per_batch, wgcs_gro_buf* bufs, wgcs_gro_call* calls,
                              wgcs_write_group* groups, int32_t* n_groups, int32_t* status, hipStream_t s) {
  if (n_batches == 0) return hipSuccess;
  const uint32_t blocks = (n_batches + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(write_build_kernel, dim3(blocks), dim3(kThreads), 0, s, pkts, verdict, n_msgs, n_batches, key_peer,
                     n_keys, offset, cap, gro_flags, calls_per_batch, bufs, calls, groups, n_groups, status);
  return hipGetLastError();
}

}  // namespace wgcs
