// staged.cpp -- the staged queue on host memory (include/wgcsum.h), no context and no device:
//   wgcs_staged_stage_host     StagePackets and the re-staging of :402-407   device/send.go:331-350
//   wgcs_staged_release_host   SendStagedPackets up to the nonce loop        send.go:363-426
//   wgcs_staged_flush_host     FlushStagedPackets                            send.go:352-361
// They run the row functions of wgcs_staged.h, the code the lanes of staged_kernels.hip run,
// taken in row order; the stage form orders the jobs by (peer row, job) with a sort of its own
// in the caller's scratch.  Plain C++: the host test program (tests/staged_host/staged_host.cpp)
// links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include <algorithm>

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_staged.h"

using namespace wgcs;

namespace {

inline bool rings_ok(const uint32_t* len, const uint32_t* head, const int32_t* slot_size, const uint8_t* ring,
                     uint32_t n_peers, uint32_t cap, uint64_t stride) {
  return n_peers <= kMaxPeers && staged_shape_ok(n_peers, cap, stride) && (!n_peers || (len && head && slot_size && ring));
}

}  // namespace

extern "C" {

int wgcs_staged_stage_host(const uint8_t* arena, uint64_t stride, const int32_t* sizes, const uint32_t* peer,
                           const int32_t* count, const int32_t* status_in, const int32_t* status_out,
                           const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, const uint32_t* peer_rows,
                           uint32_t n_ids, uint32_t* len, uint32_t* head, uint32_t* lost, int32_t* slot_size,
                           uint8_t* ring, uint32_t n_peers, uint32_t cap, uint32_t* where, void* work,
                           size_t work_bytes) {
  if (n_jobs == 0) return WGCS_OK;
  if (!arena || !sizes || !peer || !count || !status_in || !status_out || !job_key || !where || !work ||
      (n_ids && !peer_rows) || (n_peers && !lost) || !rings_ok(len, head, slot_size, ring, n_peers, cap, stride))
    return WGCS_ERR_INVALID_ARG;
  if (n_jobs > kKeyOrderMaxRows || max_segs == 0 || (uint64_t)n_jobs * max_segs > kStagedMaxSlots ||
      work_bytes < staged_stage_host_work_bytes(n_jobs) || ((uintptr_t)work & 7))
    return WGCS_ERR_INVALID_ARG;
  uint64_t* const place = (uint64_t*)work;
  uint32_t* const keys = (uint32_t*)(place + n_jobs);
  uint32_t* const order = keys + n_jobs;
  const uint32_t n_rows = n_jobs * max_segs;
  // the launches of the device form, each a loop: keys, the key order, the groups, the copy
  for (uint32_t q = 0; q < n_rows; ++q) where[q] = WGCS_STAGED_NONE;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    const uint32_t row =
        staged_job_row(j, peer, count, status_in, status_out, job_key, max_segs, peer_rows, n_ids, n_peers);
    const uint32_t nv = row != WGCS_PEER_NONE ? staged_segs_ok(j, (uint32_t)count[j], sizes, max_segs, stride) : 0;
    keys[j] = nv ? row : n_peers;
    order[j] = j;
    place[j] = nv;
  }
  std::sort(order, order + n_jobs,
            [keys](uint32_t a, uint32_t b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a < b; });
  for (uint32_t p0 = 0; p0 < n_jobs && keys[order[p0]] < n_peers;) {
    const uint32_t r = keys[order[p0]];
    uint32_t p1 = p0, m = 0;
    for (; p1 < n_jobs && keys[order[p1]] == r; ++p1) m += (uint32_t)place[order[p1]];
    const StagedGroup g = staged_group(len[r], head[r], m, cap);
    uint32_t k0 = 0;
    for (uint32_t p = p0; p < p1; ++p) {
      const uint32_t nv = (uint32_t)place[order[p]];
      place[order[p]] = staged_place(g, k0, nv, cap);
      k0 += nv;
    }
    head[r] = g.head;
    len[r] = g.len;
    lost[r] += g.evicted;
    p0 = p1;
  }
  for (uint32_t q = 0; q < n_rows; ++q) {
    const uint32_t j = q / max_segs, r = keys[j];
    if (r >= n_peers) continue;
    const uint32_t w = staged_seg_where(j, q - j * max_segs, sizes, count, max_segs, stride, r, place[j], cap);
    if (w == WGCS_STAGED_NONE) continue;
    where[q] = w;
    if (w == WGCS_STAGED_EVICTED) continue;
    slot_size[w] = sizes[q];
    memcpy(ring + (uint64_t)w * stride + kStagedHead, arena + (uint64_t)q * stride + kStagedHead, (size_t)sizes[q]);
  }
  return WGCS_OK;
}

int wgcs_staged_release_host(int64_t now_ns, const wgcs_peer_key* table, const wgcs_keypairs* kp,
                             const uint64_t* send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey,
                             uint32_t* len, uint32_t* head, const int32_t* slot_size, const uint8_t* ring,
                             uint32_t n_peers, uint32_t cap, uint64_t stride, uint32_t n_out_max, uint8_t* out,
                             uint32_t* out_peer, int32_t* out_count, int32_t* out_sizes, int32_t* out_status,
                             uint32_t* n_out, int32_t* status) {
  if (!n_out || (n_peers && (!table || !kp || !rekey || !status)) || (n_keys && !send_nonce) ||
      (n_out_max && (!out || !out_peer || !out_count || !out_sizes || !out_status)) || n_out_max > kStagedMaxSlots ||
      !rings_ok(len, head, slot_size, ring, n_peers, cap, stride))
    return WGCS_ERR_INVALID_ARG;
  // the passes of the device form: verdicts, the candidates by the weight below them, the copy, the tail
  for (uint32_t r = 0; r < n_peers; ++r)
    status[r] = staged_release_verdict(r, now_ns, len, kp, send_nonce, n_keys, limit, rekey);
  uint64_t weight = 0;
  for (uint32_t r = 0; r < n_peers; ++r)
    if (status[r] == WGCS_STAGED_RELEASED) weight += len[r];
  *n_out = weight < n_out_max ? (uint32_t)weight : n_out_max;
  uint32_t P = 0;
  for (uint32_t r = 0; r < n_peers; ++r) {
    if (status[r] != WGCS_STAGED_RELEASED) continue;
    const uint32_t w = len[r];
    uint32_t base = kStagedNoBase;
    status[r] = staged_release_commit(0, P, w, n_out_max, &base, n_out);
    if (base != kStagedNoBase) {
      for (uint32_t i = 0; i < w; ++i) {
        const uint32_t slot = r * cap + ((head[r] + i) & (cap - 1)), k = P + i;
        const int32_t size = staged_slot_size(slot_size[slot], stride);
        staged_out_row(k, table[r].peer, size, out_peer, out_count, out_sizes, out_status);
        memcpy(out + (uint64_t)k * stride + kStagedHead, ring + (uint64_t)slot * stride + kStagedHead, (size_t)size);
      }
      len[r] = 0;
      head[r] = 0;
    }
    P += w;
  }
  for (uint32_t k = *n_out; k < n_out_max; ++k) staged_out_tail(k, out_peer, out_count, out_sizes, out_status);
  return WGCS_OK;
}

int wgcs_staged_flush_host(const uint32_t* actions, uint32_t* len, uint32_t* head, uint32_t* lost, uint32_t n_peers) {
  if (n_peers == 0) return WGCS_OK;
  if (!len || !head || !lost || n_peers > kMaxPeers) return WGCS_ERR_INVALID_ARG;
  for (uint32_t r = 0; r < n_peers; ++r) staged_flush_row(r, actions, len, head, lost);
  return WGCS_OK;
}

}  // extern "C"
