// endpoint_api.cpp -- C ABI of the peer endpoints on device-resident tables
// (include/wgcsum.h):
//   wgcs_endpoint_recv_batch            the endpoint of every slot of a receive batch   conn/bind.go:308-319
//   wgcs_endpoint_set_received_batch    SetEndpointFromPacket behind write_build        device/receive.go:487
//   wgcs_endpoint_set_accepted_batch    ... behind accept                               :314
//   wgcs_endpoint_set_finished_batch    ... behind finish                               :335
//   wgcs_endpoint_dst_jobs_batch        Peer.Send up to bind.Send for send jobs         device/peer.go:201-211
//   wgcs_endpoint_dst_initiated_batch   ... for initiations
//   wgcs_endpoint_dst_responded_batch   ... for responses
// They run the bodies of wgcs_endpoint.h through launch_each; every table is the
// caller's device memory.
// The argument rules are those of the host forms (endpoint.cpp), shared through
// wgcs_endpoint.h.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_endpoint.h"
#include "wgcs_kernels.h"

using namespace wgcs;

namespace {

const char kSetArgs[] =
    "NULL, misaligned or overlapping d_ep / d_table / d_claim / d_timers, or n_rows > 2^28, n_peers > 2^24";
const char kDstArgs[] =
    "NULL, misaligned or overlapping d_table / d_timers / d_dst / d_dst_v6 / d_dst_status / d_tx_bytes, or a count "
    "over its bound";

// claim, then commit: the two launches of a set call
template <class Rows>
hipError_t launch_set(const Rows& src, uint32_t n, const wgcs_endpoint* ep, uint32_t n_rows, wgcs_endpoint* table,
                      uint32_t* claim, wgcs_timers* timers, hipStream_t s) {
  return launch_each(EndpointSetClaim<Rows>{src, ep, n_rows, claim},
                     EndpointSetCommit<Rows>{src, ep, n_rows, table, claim, timers}, n, s);
}

// read, then clear: the two launches of a dst call over descriptors
template <class Rows>
hipError_t launch_dst(const Rows& src, uint32_t n, wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst,
                      int32_t* dst_v6, int32_t* dst_status, hipStream_t s) {
  return launch_each(EndpointDstRead<Rows>{src, table, timers, dst, dst_v6, dst_status},
                     EndpointDstClear<Rows>{src, table, timers}, n, s);
}

}  // namespace

extern "C" {

int wgcs_endpoint_recv_batch(wgcs_ctx* ctx, const wgcs_src_addr* d_addr, const int32_t* d_from, const int32_t* d_size,
                             const uint8_t* d_oob, uint32_t oob_stride, const int32_t* d_nn, uint32_t n_msgs,
                             uint32_t n_batches, wgcs_endpoint* d_ep, wgcs_src_addr* d_addr_out, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)n_batches * n_msgs;
  if (n == 0) return WGCS_OK;
  if (!endpoint_recv_args_ok(d_addr, d_from, d_size, d_oob, oob_stride, d_nn, n, d_ep, d_addr_out))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "NULL, misaligned or overlapping argument, oob_stride no multiple of 4, or more than 2^28 slots");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const EndpointRecv body = {n_msgs, d_addr, d_from, d_size, d_oob, oob_stride, d_nn, d_ep, d_addr_out};
  const hipError_t e = launch_each(body, (uint32_t)n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_recv launch");
}

int wgcs_endpoint_set_received_batch(wgcs_ctx* ctx, const wgcs_write_group* d_groups, uint32_t n_batches,
                                     uint32_t calls_per_batch, const wgcs_endpoint* d_ep, uint32_t n_rows,
                                     const uint32_t* d_peer_rows, uint32_t n_ids, wgcs_endpoint* d_table,
                                     uint32_t* d_claim, wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !d_groups || misaligned(d_groups, 7) || (n_ids && !d_peer_rows) || misaligned(d_peer_rows, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n_batches * calls_per_batch <= 2^28, 8-byte aligned d_groups, 4-byte aligned d_peer_rows");
  if (!endpoint_set_tables_ok(d_ep, n_rows, d_table, d_claim, d_timers, n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kSetArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_set(GroupRows{d_groups, d_peer_rows, n_ids, n_peers}, (uint32_t)n, d_ep, n_rows, d_table,
                                  d_claim, d_timers, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_set_received launch");
}

int wgcs_endpoint_set_accepted_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, uint32_t n_tickets,
                                     const wgcs_endpoint* d_ep, uint32_t n_rows, wgcs_endpoint* d_table,
                                     uint32_t* d_claim, wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_tickets == 0) return WGCS_OK;
  if (n_tickets > kMaxRows || !d_resp || misaligned(d_resp, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_tickets <= 2^28, 4-byte aligned d_resp");
  if (!endpoint_set_tables_ok(d_ep, n_rows, d_table, d_claim, d_timers, n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kSetArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_set(AcceptedRows{d_resp, n_peers}, n_tickets, d_ep, n_rows, d_table, d_claim, d_timers,
                                  stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_set_accepted launch");
}

int wgcs_endpoint_set_finished_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                                     const int32_t* d_gate, uint32_t n, const wgcs_session_slot* d_hs_slots,
                                     uint32_t n_hs_slots, const wgcs_hs_state* d_states, uint32_t n_states,
                                     const wgcs_endpoint* d_ep, wgcs_endpoint* d_table, uint32_t* d_claim,
                                     wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_gate || (n_hs_slots && !d_hs_slots) || (n_states && !d_states))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxPeers || !pow2_or_0(n_hs_slots) || misaligned(d_pkts, 7) || misaligned(d_gate, 3) ||
      misaligned(d_hs_slots, 3) || misaligned(d_states, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^24, n_hs_slots 0 or a power of two, 8-byte aligned d_pkts, 4-byte aligned rows");
  if (!endpoint_set_tables_ok(d_ep, n, d_table, d_claim, d_timers, n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kSetArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const FinishedRows src = {d_arena, d_pkts, d_gate, d_hs_slots, n_hs_slots, d_states, n_states, n_peers};
  const hipError_t e =
      launch_set(src, n, d_ep, n, d_table, d_claim, d_timers, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_set_finished launch");
}

int wgcs_endpoint_dst_jobs_batch(wgcs_ctx* ctx, const uint32_t* d_peer, const int32_t* d_count, const int32_t* d_status,
                                 const uint32_t* d_job_key, uint32_t n_jobs, uint32_t max_segs, const int32_t* d_lens,
                                 int32_t* d_nbufs, const uint32_t* d_peer_rows, uint32_t n_ids, wgcs_endpoint* d_table,
                                 wgcs_timers* d_timers, uint32_t n_peers, wgcs_endpoint* d_dst, int32_t* d_dst_v6,
                                 int32_t* d_dst_status, uint64_t* d_tx_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_peer || !d_count || !d_status || !d_job_key || !d_lens || !d_nbufs || (n_ids && !d_peer_rows))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (max_segs == 0 || (uint64_t)n_jobs * max_segs > kMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "max_segs >= 1, n_jobs * max_segs <= 2^28");
  if (misaligned(d_peer, 3) || misaligned(d_count, 3) || misaligned(d_status, 3) || misaligned(d_job_key, 3) ||
      misaligned(d_lens, 3) || misaligned(d_nbufs, 3) || misaligned(d_peer_rows, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned job arrays");
  if (!endpoint_dst_tables_ok(n_jobs, d_table, d_timers, n_peers, d_dst, d_dst_v6, d_dst_status, d_tx_bytes, true))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kDstArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const KeptJobRows src = {{d_peer, d_count, d_status, max_segs, d_peer_rows, n_ids, n_peers}, d_job_key};
  const hipError_t e = launch_each(
      EndpointDstJobs{{src, d_table, d_timers, d_dst, d_dst_v6, d_dst_status}, d_lens, d_nbufs, d_tx_bytes},
      EndpointDstClear<KeptJobRows>{src, d_table, d_timers}, n_jobs, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_dst_jobs launch");
}

int wgcs_endpoint_dst_initiated_batch(wgcs_ctx* ctx, const wgcs_hs_start* d_start, const int32_t* d_status, uint32_t n,
                                      wgcs_endpoint* d_table, wgcs_timers* d_timers, uint32_t n_peers,
                                      wgcs_endpoint* d_dst, int32_t* d_dst_v6, int32_t* d_dst_status, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_start || !d_status || misaligned(d_start, 3) || misaligned(d_status, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_start and d_status: not NULL, 4-byte aligned");
  if (!endpoint_dst_tables_ok(n, d_table, d_timers, n_peers, d_dst, d_dst_v6, d_dst_status, nullptr, false))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kDstArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_dst(InitiatedRows{d_start, d_status, n_peers}, n, d_table, d_timers, d_dst, d_dst_v6,
                                  d_dst_status, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_dst_initiated launch");
}

int wgcs_endpoint_dst_responded_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, const int32_t* d_status, uint32_t n,
                                      wgcs_endpoint* d_table, wgcs_timers* d_timers, uint32_t n_peers,
                                      wgcs_endpoint* d_dst, int32_t* d_dst_v6, int32_t* d_dst_status, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_resp || !d_status || misaligned(d_resp, 3) || misaligned(d_status, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_resp and d_status: not NULL, 4-byte aligned");
  if (!endpoint_dst_tables_ok(n, d_table, d_timers, n_peers, d_dst, d_dst_v6, d_dst_status, nullptr, false))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, kDstArgs);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_dst(RespondedRows{d_resp, d_status, n_peers}, n, d_table, d_timers, d_dst, d_dst_v6,
                                  d_dst_status, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "endpoint_dst_responded launch");
}

}  // extern "C"
