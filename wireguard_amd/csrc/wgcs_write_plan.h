// wgcs_write_plan.h -- the Write calls of one receive batch, one per peer, as
// scalar code: which rows of a batch RoutineSendToInternet sees, how they fall
// into per-peer groups, and the wgcs_gro_buf / wgcs_gro_call / wgcs_write_group
// rows that result (device/receive.go:178-228, :398-504).  Shared by the host
// entry point (write_api.cpp), the stand-alone sanitizer program of
// tests/write_host/ and, row rules and row images alike, the wave form of
// write_kernels.hip, which must reproduce write_plan_batch array for array.
//
// RoutineReceiveIncoming sorts the items of a recvmmsg batch into one
// container per peer (:178-186, :220-228); each peer's RoutineSendToInternet
// runs the replay filter over its container in slot order, does the peer's
// bookkeeping for every message that passes (:407-436) and hands the packets
// that also pass the length and source checks to one Tun.Write (:483-504).
// Go leaves the order of the peers open (map iteration, a goroutine each);
// here a batch's groups are ordered by each peer's first validated row.
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WGCS_WRITE_HD __host__ __device__ inline
#else
#define WGCS_WRITE_HD inline
#endif

namespace wgcs {

constexpr uint32_t kWriteMaxRows = WGCS_GRO_MAX_CALL;  // conn.BatchSize: rows of a batch, and so its groups
constexpr uint64_t kWriteMaxTable = 1ull << 28;        // rows of the whole table are counted in 32 bits
constexpr uint32_t kMinMessageSize = 32;               // MessageTransportSize: a longer message carries data (:436)

static_assert(sizeof(wgcs_write_group) == 24, "wgcs_write_group layout");
static_assert(sizeof(wgcs_gro_buf) == 16 && sizeof(wgcs_gro_call) == 16, "GRO row layout");

// The peer whose RoutineSendToInternet validated row q, or WGCS_PEER_NONE for
// a row that takes no part: wgcs_replay_batch's participation rule (a listed
// key and a message Open decrypted) minus the filter's rejects; a source
// verdict is one that passed the filter first.  key_peer is read for a listed
// key only.
WGCS_WRITE_HD uint32_t write_row_peer(uint32_t key, int32_t verdict, const uint32_t* key_peer, uint32_t n_keys) {
  if (key >= n_keys) return WGCS_PEER_NONE;
  if (!(verdict >= 0 || verdict == WGCS_ERR_SOURCE || verdict == WGCS_ERR_PACKET_TOO_SHORT)) return WGCS_PEER_NONE;
  return key_peer[key];
}

// a validated row that reaches Tun.Write (:483)
WGCS_WRITE_HD bool write_row_kept(uint32_t peer, int32_t verdict) { return peer != WGCS_PEER_NONE && verdict > 0; }

// elem.buffer[:offset + len(packet)] of a kept row is a slice Go can make
WGCS_WRITE_HD bool write_row_fits(int32_t offset, int32_t verdict, uint32_t cap) {
  return (int64_t)offset + (int64_t)verdict <= (int64_t)cap;
}

WGCS_WRITE_HD bool write_row_data(uint32_t msg_len) { return msg_len > kMinMessageSize; }

WGCS_WRITE_HD wgcs_gro_buf write_buf_row(uint64_t off, int32_t offset, int32_t verdict, uint32_t cap) {
  wgcs_gro_buf r;
  r.off = off;
  r.len = (uint32_t)offset + (uint32_t)verdict;
  r.cap = cap;
  return r;
}

WGCS_WRITE_HD wgcs_gro_buf write_buf_zero() {
  wgcs_gro_buf r;
  r.off = 0;
  r.len = 0;
  r.cap = 0;
  return r;
}

WGCS_WRITE_HD wgcs_gro_call write_call_row(uint32_t first, uint32_t n, int32_t offset, uint32_t gro_flags) {
  wgcs_gro_call r;
  r.first = first;
  r.n = n;
  r.offset = offset;
  r.flags = gro_flags;
  return r;
}

WGCS_WRITE_HD wgcs_write_group write_group_unused() {
  wgcs_write_group r;
  r.peer = WGCS_PEER_NONE;
  r.tail = -1;
  r.flags = 0;
  r.n_valid = 0;
  r.rx_bytes = 0;
  return r;
}

// the scalar arguments both entry points accept
WGCS_WRITE_HD bool write_args_ok(uint32_t n_msgs, uint32_t n_batches, int32_t offset, uint32_t cap,
                                 uint32_t calls_per_batch) {
  return n_msgs >= 1 && n_msgs <= kWriteMaxRows && calls_per_batch >= 1 && calls_per_batch <= n_msgs &&
         (uint64_t)n_batches * n_msgs <= kWriteMaxTable && offset >= 0 && (uint64_t)offset <= cap;
}

// Batch b of the table.  pkts / verdict / bufs are the whole arrays (batch b
// owns rows [b * n_msgs, (b + 1) * n_msgs)), calls / groups likewise (rows
// [b * calls_per_batch, (b + 1) * calls_per_batch)).  Every row the batch owns
// is written, whatever becomes of it.  Returns the batch's status.
WGCS_WRITE_HD int32_t write_plan_batch(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t b, uint32_t n_msgs,
                                       const uint32_t* key_peer, uint32_t n_keys, int32_t offset, uint32_t cap,
                                       uint32_t gro_flags, uint32_t calls_per_batch, wgcs_gro_buf* bufs,
                                       wgcs_gro_call* calls, wgcs_write_group* groups, int32_t* n_groups) {
  const uint32_t q0 = b * n_msgs;
  const wgcs_aead_pkt* pk = pkts + q0;
  const int32_t* vd = verdict + q0;
  wgcs_gro_buf* bf = bufs + q0;
  wgcs_gro_call* cl = calls + (uint64_t)b * calls_per_batch;
  wgcs_write_group* gr = groups + (uint64_t)b * calls_per_batch;
  uint32_t peer[kWriteMaxRows];
  int16_t group_of[kWriteMaxRows];  // -1: none yet
  bool fits = true;
  for (uint32_t i = 0; i < n_msgs; ++i) {
    peer[i] = write_row_peer(pk[i].key, vd[i], key_peer, n_keys);
    group_of[i] = -1;
    if (write_row_kept(peer[i], vd[i]) && !write_row_fits(offset, vd[i], cap)) fits = false;
  }
  // groups in the order of their first validated row
  uint32_t ng = 0;
  for (uint32_t i = 0; i < n_msgs; ++i) {
    if (peer[i] == WGCS_PEER_NONE || group_of[i] >= 0) continue;
    for (uint32_t j = i; j < n_msgs; ++j)
      if (peer[j] == peer[i]) group_of[j] = (int16_t)ng;
    ++ng;
  }
  *n_groups = (int32_t)ng;
  const int32_t status = !fits ? WGCS_ERR_OUT_OF_RANGE : ng > calls_per_batch ? WGCS_ERR_BATCH_FULL : WGCS_OK;
  const uint32_t used = status == WGCS_OK ? ng : 0;
  uint32_t kept_total = 0;
  for (uint32_t g = 0; g < used; ++g) {
    wgcs_write_group w = write_group_unused();
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_msgs; ++i) {
      if (group_of[i] != (int16_t)g) continue;
      w.peer = peer[i];
      w.tail = (int32_t)(q0 + i);
      if (write_row_data(pk[i].len)) w.flags |= WGCS_GROUP_DATA;
      ++w.n_valid;
      w.rx_bytes += pk[i].len;
      if (write_row_kept(peer[i], vd[i])) bf[kept_total + n++] = write_buf_row(pk[i].off, offset, vd[i], cap);
    }
    cl[g] = write_call_row(q0 + kept_total, n, offset, gro_flags);
    gr[g] = w;
    kept_total += n;
  }
  for (uint32_t g = used; g < calls_per_batch; ++g) {
    cl[g] = write_call_row(q0, 0, offset, gro_flags);
    gr[g] = write_group_unused();
  }
  for (uint32_t i = kept_total; i < n_msgs; ++i) bf[i] = write_buf_zero();
  return status;
}

}  // namespace wgcs
