// wgcs_staged.h -- the staged queue (peer.qus.staged) as scalar row functions, shared by
// host and device:
//   StagePackets         device/send.go:331-350, and the re-staging of :402-407
//   FlushStagedPackets   send.go:352-361
//   SendStagedPackets    send.go:363-426 up to the nonce loop, which is send-assign's
// staged_kernels.hip runs them one lane (or one 16-lane group) per row, staged.cpp in row
// order, and the stand-alone sanitizer program of tests/staged_host/ includes this one text.
//
// The state is that of include/wgcsum.h: per peer row r a ring of cap packet slots, slot
// s = r * cap + pos with its packet at s * stride + 16, and the words len[r], head[r], lost[r].
// The unit is the packet.  A call's new packets of one peer are ranked 0 .. m - 1 in job order,
// then segment order; everything a packet needs to find its slot is its rank, the ring's tail
// before the call and m, so no packet waits for another.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/wgcsum.h"
#include "wgcs_rekey.h"

namespace wgcs {

constexpr uint32_t kStagedMaxCap = 1024;         // ring slots of a peer
constexpr uint32_t kStagedMaxSlots = 1u << 28;   // n_peers * cap, and n_jobs * max_segs
constexpr uint32_t kStagedHead = 16;             // header room in front of a packet: the seal's
constexpr uint32_t kStagedRoom = 16 + 32;        // header room, and padding and tag behind the packet
constexpr uint32_t kStagedNoBase = 0xFFFFFFFFu;  // release's scratch word of a row that keeps its ring

WGCS_HD bool staged_shape_ok(uint32_t n_peers, uint32_t cap, uint64_t stride) {
  return cap >= 1 && cap <= kStagedMaxCap && (cap & (cap - 1)) == 0 && (uint64_t)n_peers * cap <= kStagedMaxSlots &&
         stride >= 16 && (stride & 15) == 0;
}

// A packet the seal can take from a slot of `stride` bytes: header, size bytes, and up to 15
// bytes of padding and the tag.  stride is a multiple of 16, so 16 + size + 32 <= stride is
// wgcs_aead_seal_batch's own 32 + padded <= stride.
WGCS_HD bool staged_seg_ok(int32_t size, uint64_t stride) { return size >= 0 && (uint64_t)size + kStagedRoom <= stride; }

// ---- stage ----

// The peer row of job j if it is to be staged, else WGCS_PEER_NONE: taken by send-assign's own
// rule on status_in, and refused by the gate or dropped by send-assign.
WGCS_HD uint32_t staged_job_row(uint32_t j, const uint32_t* peer, const int32_t* count, const int32_t* status_in,
                                const int32_t* status_out, const uint32_t* job_key, uint32_t max_segs,
                                const uint32_t* peer_rows, uint32_t n_ids, uint32_t n_peers) {
  const int32_t so = status_out[j];
  if (so != WGCS_ERR_KEY_EXPIRED && !(so == 0 && job_key[j] == kRekeyNoKey)) return WGCS_PEER_NONE;
  return JobRows{peer, count, status_in, max_segs, peer_rows, n_ids, n_peers}.row(j);
}

// the packets among segments [0, s) of job j (count[j] checked by staged_job_row) that a slot can hold
WGCS_HD uint32_t staged_segs_ok(uint32_t j, uint32_t s, const int32_t* sizes, uint32_t max_segs, uint64_t stride) {
  const int32_t* const z = sizes + (uint64_t)j * max_segs;
  uint32_t n = 0;
  for (uint32_t i = 0; i < s; ++i) n += staged_seg_ok(z[i], stride) ? 1u : 0u;
  return n;
}

// What m new packets do to a ring of L packets at head h: rank k goes to (tail + k) & (cap - 1)
// unless k < drop, and the row's words become head, len and lost + evicted.
struct StagedGroup {
  uint32_t tail, drop, head, len, evicted;
};
WGCS_HD StagedGroup staged_group(uint32_t L, uint32_t h, uint32_t m, uint32_t cap) {
  const uint32_t mask = cap - 1;
  h &= mask;
  if (L > cap) L = cap;
  const uint32_t total = L + m;  // m <= 2^28
  StagedGroup g;
  g.evicted = total > cap ? total - cap : 0;  // the oldest go first: old ones, then this call's own
  g.drop = m > cap ? m - cap : 0;
  g.tail = (h + L) & mask;
  g.head = (h + g.evicted) & mask;
  g.len = total - g.evicted;
  return g;
}

// A job's share of its group as one word: the position of its first packet (rank k0) in the low
// half, and in the high half how many of its nv packets, from the front, the call itself evicts.
WGCS_HD uint64_t staged_place(const StagedGroup& g, uint32_t k0, uint32_t nv, uint32_t cap) {
  uint32_t ev = g.drop > k0 ? g.drop - k0 : 0;
  if (ev > nv) ev = nv;
  return (uint64_t)((g.tail + k0) & (cap - 1)) | ((uint64_t)ev << 32);
}

// Slot q = j * max_segs + s of a staged job of peer row r: the ring slot its packet goes to,
// WGCS_STAGED_NONE for a slot that carries no packet a ring slot can hold, WGCS_STAGED_EVICTED
// for one that m - cap later packets of the call pushed out before it was ever copied.
WGCS_HD uint32_t staged_seg_where(uint32_t j, uint32_t s, const int32_t* sizes, const int32_t* count, uint32_t max_segs,
                                  uint64_t stride, uint32_t r, uint64_t place, uint32_t cap) {
  if ((int32_t)s >= count[j]) return WGCS_STAGED_NONE;
  if (!staged_seg_ok(sizes[(uint64_t)j * max_segs + s], stride)) return WGCS_STAGED_NONE;
  const uint32_t idx = staged_segs_ok(j, s, sizes, max_segs, stride);
  if (idx < (uint32_t)(place >> 32)) return WGCS_STAGED_EVICTED;
  return r * cap + (((uint32_t)place + idx) & (cap - 1));
}

// ---- release ----

// send.go:365-374 for peer row r: WGCS_HS_NONE for an empty queue, WGCS_ERR_KEY_EXPIRED (and the
// reasons OR-ed into want) for a current keypair that cannot send, else WGCS_STAGED_RELEASED for
// a candidate, which the commit confirms or turns into WGCS_ERR_BATCH_FULL.
WGCS_HD int32_t staged_release_verdict(uint32_t r, int64_t now, const uint32_t* len, const wgcs_keypairs* kp,
                                       const uint64_t* send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey) {
  if (len[r] == 0) return WGCS_HS_NONE;
  const uint32_t w = rekey_gate_want(r, now, kp, send_nonce, n_keys, limit);
  if (w == 0) return WGCS_STAGED_RELEASED;
  rekey_want_or(rekey + r, w);
  return WGCS_ERR_KEY_EXPIRED;
}

// The candidate r of weight w = len[r] that candidates of weight P in all precede: base[r] = P
// if its packets fit the budget, else the row keeps its ring; the first that does not fit is
// where the job table ends.
WGCS_HD int32_t staged_release_commit(uint32_t r, uint32_t P, uint32_t w, uint32_t n_out_max, uint32_t* base,
                                      uint32_t* n_out) {
  if ((uint64_t)P + w <= n_out_max) {
    base[r] = P;
    return WGCS_STAGED_RELEASED;
  }
  base[r] = kStagedNoBase;
  if (P <= n_out_max) *n_out = P;  // every candidate below fitted, and none past this one does: P only grows
  return WGCS_ERR_BATCH_FULL;
}

// The size word of a ring slot as the copy takes it: stage writes only sizes a slot can hold, and
// a word that is none (the state is the caller's memory) moves no byte.
WGCS_HD int32_t staged_slot_size(int32_t size, uint64_t stride) { return staged_seg_ok(size, stride) ? size : 0; }

// job k of the output table: one packet of `size` bytes for `peer`
WGCS_HD void staged_out_row(uint32_t k, uint32_t peer, int32_t size, uint32_t* out_peer, int32_t* out_count,
                            int32_t* out_sizes, int32_t* out_status) {
  out_peer[k] = peer;
  out_count[k] = 1;
  out_sizes[k] = size;
  out_status[k] = 0;
}

// job k past the count: send-assign drops it by its count
WGCS_HD void staged_out_tail(uint32_t k, uint32_t* out_peer, int32_t* out_count, int32_t* out_sizes,
                             int32_t* out_status) {
  out_peer[k] = WGCS_PEER_NONE;
  out_count[k] = 0;
  out_sizes[k] = 0;
  out_status[k] = 0;
}

// ---- flush ----

// send.go:352-361 for peer row r; actions == NULL is peer.Stop's flush of every row
WGCS_HD void staged_flush_row(uint32_t r, const uint32_t* actions, uint32_t* len, uint32_t* head, uint32_t* lost) {
  if (actions && !(actions[r] & WGCS_TIMERS_ACT_FLUSH_STAGED)) return;
  lost[r] += len[r];
  len[r] = 0;
  head[r] = 0;
}

// ---- the host forms' scratch (staged.cpp) ----

// stage: place (8 B), key and order (4 B each) per job, 8-byte aligned; wgcs_keyorder_work_bytes(n_jobs) covers it
WGCS_HD size_t staged_stage_host_work_bytes(uint32_t n_jobs) { return (size_t)16 * n_jobs; }

}  // namespace wgcs
