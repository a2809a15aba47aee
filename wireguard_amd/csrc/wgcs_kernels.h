// wgcs_kernels.h -- host-side launch entry points of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_batch_plan.h"
#include "wgcs_host.h"

namespace wgcs {

hipError_t launch_checksum_batch(int mode, unsigned flags, uint8_t* arena, const wgcs_pkt* pkts,
                                 const uint64_t* init, uint32_t n, void* out, hipStream_t s, int num_cu,
                                 const LaunchTuning& tune);
// One launch for a group of batches (wgcs_batch_plan.h; never in place), and
// the packets one block covers per grid-stride step, which the plan needs.
hipError_t launch_checksum_group(int mode, const BatchTable& tab, hipStream_t s, const LaunchTuning& tune);
int checksum_pkts_per_block(const LaunchTuning& tune);

// the resident per-call ring (ring_kernels.hip): nb workgroups serve the
// requests of ctl (coherent pinned host memory) until its stop word or
// idle_ticks (100 MHz) without a request
hipError_t launch_ring(RingCtl* ctl, uint32_t nb, uint32_t last, uint64_t idle_ticks, hipStream_t s);
void gso_kernel_shape(int* lds_waves, int* parts, int* u, int* rows);
hipError_t launch_gso_split_batch(const uint8_t* arena, const wgcs_gso_job* jobs, uint32_t n_jobs,
                                  uint8_t* out, uint32_t out_stride, uint32_t offset, uint32_t max_segs,
                                  int32_t* sizes, int32_t* count, int32_t* status,
                                  hipStream_t s, const GsoOutPos* outpos = nullptr, uint32_t room = 0);

// Device-resident batch of handleGRO calls (gro_batch_kernels.hip).
hipError_t launch_gro_batch(uint8_t* arena, wgcs_gro_buf* bufs, const wgcs_gro_call* calls, uint32_t n_calls,
                            int32_t* status, int32_t* n_write, int32_t* to_write, hipStream_t s);

hipError_t launch_ws_scatter(const uint8_t* stage, uint8_t* arena, const WsMove* mv, uint32_t n, hipStream_t s);
hipError_t launch_ws_gather(const uint8_t* arena, const wgcs_gro_buf* bufs, const wgcs_gro_call* calls,
                            const WsOut* outs, uint32_t n_calls, int32_t* status, const int32_t* n_write,
                            const int32_t* to_write, int32_t* wlen, int32_t* wpos, uint8_t* out, hipStream_t s);

hipError_t launch_gro_coalesce(const uint8_t* stage, const GroItem* items, uint32_t n_items, const GroSeg* segs,
                               uint32_t n_segs, uint8_t* out, hipStream_t s);

// Outer-UDP message batching (conn/bind.go:542-662), udp_msgs_kernels.hip.
hipError_t launch_udp_split(const uint8_t* in, uint64_t in_stride, uint32_t buf_len, const int32_t* n_in,
                            const int32_t* gso, uint32_t n_msgs, uint32_t first, uint32_t n_batches, uint8_t* out,
                            uint64_t out_stride, int32_t* n_out, int32_t* src, int32_t* count, int32_t* status,
                            hipStream_t s);
hipError_t launch_udp_coalesce(uint8_t* bufs, uint64_t stride, uint32_t buf_cap, const int32_t* caps,
                               const int32_t* lens, const int32_t* nbufs, uint32_t max_bufs, uint32_t n_batches,
                               int dst_is_v6, int32_t* n_msgs, int32_t* msg_first, int32_t* msg_len,
                               int32_t* msg_gso, hipStream_t s);
// the same with the family of batch b in dst_v6[b]: the kernel's other instantiation
hipError_t launch_udp_coalesce_dst(uint8_t* bufs, uint64_t stride, uint32_t buf_cap, const int32_t* caps,
                                   const int32_t* lens, const int32_t* nbufs, uint32_t max_bufs, uint32_t n_batches,
                                   const int32_t* dst_v6, int32_t* n_msgs, int32_t* msg_first, int32_t* msg_len,
                                   int32_t* msg_gso, hipStream_t s);

// Transport AEAD, in place (aead_kernels.hip): open != 0 is Open (out_ctr
// required, mtu unused), else Seal.
hipError_t launch_aead_batch(int open, uint8_t* arena, const wgcs_aead_pkt* pkts, const wgcs_aead_key* keys,
                             uint32_t n_keys, uint32_t n, uint32_t mtu, int32_t* out_len, uint64_t* out_ctr,
                             hipStream_t s);

// Peer lookup (route_kernels.hip): receive classification against the session
// slots, the allowed-source check and destination routing against a router
// image (wgcs_route_walk.h).  off == nullptr: slot q at q * stride.
hipError_t launch_recv_classify(const uint8_t* arena, const uint64_t* off, uint64_t stride, const int32_t* sizes,
                                uint32_t n, const wgcs_session_slot* slots, uint32_t n_slots, wgcs_aead_pkt* pkts,
                                int32_t* types, hipStream_t s);
hipError_t launch_recv_source(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* pkt_len,
                              const uint32_t* key_peer, uint32_t n_keys, uint32_t n, const uint8_t* image,
                              uint64_t image_bytes, int32_t* verdict, uint32_t* peer, hipStream_t s);
hipError_t launch_route_dst(const uint8_t* arena, const uint64_t* off, uint64_t stride, uint32_t offset,
                            const int32_t* sizes, uint32_t n, const uint8_t* image, uint64_t image_bytes,
                            uint32_t* peer, hipStream_t s);

// Per-keypair state (replay_kernels.hip) on a carved workspace (wgcs_keyorder.h):
// the replay filter over open's counters, and key and nonces of every send job.
struct KeyOrder;
hipError_t launch_replay(const KeyOrder& ko, const wgcs_aead_pkt* pkts, const int32_t* pkt_len,
                         const uint64_t* counter, uint32_t n, wgcs_replay_filter* filters, uint32_t n_keys,
                         uint64_t limit, int32_t* verdict, hipStream_t s);
hipError_t launch_send_assign(const KeyOrder& ko, const int32_t* sizes, const uint32_t* peer, const int32_t* count,
                              const int32_t* status, uint32_t n_jobs, uint32_t max_segs, uint64_t stride,
                              const wgcs_session_slot* peer_keys, uint32_t n_slots, uint64_t* send_nonce,
                              uint32_t n_keys, uint64_t limit, wgcs_aead_pkt* pkts, int32_t* nbufs, uint32_t* job_key,
                              hipStream_t s);

// The Write calls of every receive batch, one per peer (write_kernels.hip, the
// wave form of wgcs_write_plan.h): one wave per batch, one launch.
hipError_t launch_write_build(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n_msgs, uint32_t n_batches,
                              const uint32_t* key_peer, uint32_t n_keys, int32_t offset, uint32_t cap,
                              uint32_t gro_flags, uint32_t calls_per_batch, wgcs_gro_buf* bufs, wgcs_gro_call* calls,
                              wgcs_write_group* groups, int32_t* n_groups, int32_t* status, hipStream_t s);

// The handshake screen (cookie_kernels.hip): MAC1, and under load MAC2 and the
// cookie reply, for the rows that classify typed 1 or 2.
hipError_t launch_hs_screen(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types, uint32_t n,
                            const wgcs_cookie_checker* checker, const wgcs_src_addr* srcs, uint32_t under_load,
                            const uint8_t* nonces, int32_t* verdict, uint8_t* replies, hipStream_t s);

// Curve25519 and the consumption of screened initiations (noise_kernels.hip):
// one lane per row; gate may be NULL.
hipError_t launch_x25519(const uint8_t* scalars, const uint8_t* points, uint32_t n, uint8_t* out, int32_t* status,
                         hipStream_t s);
hipError_t launch_hs_consume(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types,
                             const int32_t* gate, uint32_t n, const wgcs_noise_responder* responder,
                             const wgcs_peer_key* table, uint32_t n_peers, int32_t* verdict, wgcs_hs_init* out,
                             hipStream_t s);
// the response to n accepted initiations, one lane per descriptor; gate and psk may be NULL
hipError_t launch_hs_respond(const wgcs_hs_resp* resp, uint32_t n, const wgcs_hs_init* init, const int32_t* gate,
                             uint32_t n_init, const wgcs_peer_key* table, const uint8_t* psk, uint32_t n_peers,
                             wgcs_aead_key* keys, uint32_t n_keys, uint8_t* msgs, int32_t* status, hipStream_t s);

// The initiator's half (noise_init_kernels.hip), one lane per row: n initiations into msgs and
// the state table, and the responses of a receive batch against that table.  launch_hs_finish
// is two launches on s, the second of which commits the lowest authentic row per handshake;
// gate and psk may be NULL.
hipError_t launch_hs_initiate(const wgcs_hs_start* start, uint32_t n, const uint8_t* static_public,
                              const wgcs_peer_key* table, uint32_t n_peers, uint32_t n_keys, wgcs_hs_state* states,
                              uint32_t n_states, uint8_t* msgs, int32_t* status, hipStream_t s);
hipError_t launch_hs_finish(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types, const int32_t* gate,
                            uint32_t n, const wgcs_noise_responder* self, const wgcs_session_slot* slots,
                            uint32_t n_slots, wgcs_hs_state* states, uint32_t n_states, const uint8_t* psk,
                            uint32_t n_peers, wgcs_aead_key* keys, uint32_t n_keys, uint8_t* work, int32_t* verdict,
                            hipStream_t s);

// The scan of a call that compacts its flagged rows (wgcs_compact.h, compact_kernels.hip): one
// block turns the n_blocks per-block counts into the counts below each block, and writes
// *count = min(their sum, cap).  launch_hs_accept, launch_rekey_start and launch_timers_expire
// each issue it between their verdict and commit launches, or in front of the commit alone when
// they have no rows; their scratch is compact_blocks(rows) words of wgcs_compact.h.
hipError_t launch_compact_scan(uint32_t* block_count, uint32_t n_blocks, uint32_t cap, uint32_t* count,
                               hipStream_t s);

// The responder's stateful tail (noise_accept_kernels.hip), one lane per row: claim, then the
// scheme of wgcs_compact.h over the winners.  The call owns block_winners until it is done.
hipError_t launch_hs_accept(const wgcs_hs_init* init, const int32_t* gate, uint32_t n, int64_t now,
                            const wgcs_peer_key* table, const uint32_t* peer_rows, uint32_t n_ids, wgcs_hs_peer* peers,
                            uint32_t n_peers, const wgcs_hs_ticket* tickets, uint32_t n_tickets, wgcs_hs_resp* resp,
                            uint32_t* count, int32_t* verdict, uint32_t* block_winners, hipStream_t s);

// Keypair rotation (keypairs_kernels.hip, the row functions of wgcs_keypairs.h).  The two begin
// forms group their descriptors by peer row on a carved workspace (wgcs_keyorder.h) and let one
// lane walk each peer's run; received is two launches, claim and commit.
hipError_t launch_keypairs_begin_responder(const KeyOrder& ko, const wgcs_hs_resp* resp, const int32_t* gate,
                                           uint32_t n, int64_t now, const wgcs_peer_key* table, uint32_t n_peers,
                                           wgcs_keypairs* kp, wgcs_session_slot* slots, uint32_t n_slots,
                                           wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys,
                                           uint32_t* key_peer, uint32_t n_keys, int32_t* status, hipStream_t s);
hipError_t launch_keypairs_begin_initiator(const KeyOrder& ko, const uint8_t* arena, const wgcs_aead_pkt* pkts,
                                           const int32_t* gate, uint32_t n, int64_t now,
                                           const wgcs_session_slot* hs_slots, uint32_t n_hs_slots,
                                           const wgcs_hs_state* states, uint32_t n_states, const wgcs_peer_key* table,
                                           uint32_t n_peers, wgcs_keypairs* kp, wgcs_session_slot* slots,
                                           uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                                           wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, int32_t* status,
                                           hipStream_t s);
hipError_t launch_keypairs_received(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n, uint32_t* key_peer,
                                    uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, wgcs_keypairs* kp,
                                    uint32_t n_peers, wgcs_session_slot* slots, uint32_t n_slots,
                                    wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys,
                                    uint32_t* rotated, hipStream_t s);

// One lane per entry (wgcs_each.h): the body f, a struct with operator()(uint32_t), for every
// i < n, and the two passes of a claim-and-commit call, the second launched behind the first on
// s.  n is not 0.  The event calls of the timers, the rekey rules, the cookie generator and the
// endpoints are such bodies (wgcs_timers.h, wgcs_rekey.h, wgcs_cookiegen.h, wgcs_endpoint.h),
// instantiated in their families' .hip files.
template <class F>
hipError_t launch_each(const F& f, uint32_t n, hipStream_t s);
template <class F, class G>
hipError_t launch_each(const F& first, const G& second, uint32_t n, hipStream_t s);

// The start of a handshake (rekey_kernels.hip, the row functions of wgcs_rekey.h): the scheme of
// wgcs_compact.h over the peer rows, the candidates flagged.
hipError_t launch_rekey_start(int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* hs_peers, uint32_t n_peers,
                              const wgcs_hs_start* tickets, uint32_t n_tickets, wgcs_hs_start* start,
                              uint32_t* start_peer, uint32_t* count, int32_t* status, uint32_t* reasons,
                              uint32_t* block_cand, hipStream_t s);

// The expiry of the peer timers (timers_kernels.hip, the row functions of wgcs_timers.h): the
// scheme of wgcs_compact.h over the peer rows, those that owe a keepalive job flagged.
hipError_t launch_timers_expire(int64_t now, wgcs_timers* timers, wgcs_rekey* rekey, const wgcs_peer_key* table,
                                uint32_t n_peers, const uint32_t* staged, wgcs_keypairs* kp, wgcs_session_slot* slots,
                                uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                                wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, uint32_t n_ka_max,
                                uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes, int32_t* ka_status,
                                uint32_t* n_ka, uint32_t* actions, uint32_t* block_owe, hipStream_t s);

// The rate limiter (ratelimit_kernels.hip, the row functions of wgcs_ratelimit.h): find or claim,
// one lane per row; the key order over the slots on a carved workspace (wgcs_keyorder.h); verdicts
// and entries, one lane per position.  stats may be NULL; n == 0 only zeroes it.  The cleanup
// zeroes new_table and *live on s, then one lane per old slot.
hipError_t launch_ratelimit(const KeyOrder& ko, const int32_t* gate, const wgcs_src_addr* src, uint32_t n,
                            wgcs_rl_entry* table, uint32_t n_slots, int64_t now, int32_t* verdict, uint32_t* stats,
                            hipStream_t s);
hipError_t launch_ratelimit_cleanup(const wgcs_rl_entry* old_table, wgcs_rl_entry* new_table, uint32_t n_slots,
                                    int64_t now, uint32_t* live, hipStream_t s);

// The staged queue (staged_kernels.hip, the row functions of wgcs_staged.h).  Stage: the jobs'
// rows as keys and a count of them, the key order over the peer rows on a carved workspace, one
// wave per peer group for the ring words and the jobs' places, then 16 lanes per slot for the
// copy; the launches behind the first exit on a zero count.  Release: the weighted form of
// wgcs_compact.h over the peer rows (scratch: its block words, then one word per peer row), then
// a block per released ring for the copy and the tail.  Flush: one lane per peer row.
struct StagedRings {  // the state of include/wgcsum.h's staged section
  uint32_t *len, *head, *lost;
  int32_t* slot_size;
  uint8_t* ring;
  uint32_t n_peers, cap;
  uint64_t stride;
};
hipError_t launch_staged_stage(const KeyOrder& ko, const uint8_t* arena, const int32_t* sizes, const uint32_t* peer,
                               const int32_t* count, const int32_t* status_in, const int32_t* status_out,
                               const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, const uint32_t* peer_rows,
                               uint32_t n_ids, const StagedRings& st, uint32_t* where, hipStream_t s);
hipError_t launch_staged_release(int64_t now, const wgcs_peer_key* table, const wgcs_keypairs* kp,
                                 const uint64_t* send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey,
                                 const StagedRings& st, uint32_t n_out_max, uint8_t* out, uint32_t* out_peer,
                                 int32_t* out_count, int32_t* out_sizes, int32_t* out_status, uint32_t* n_out,
                                 int32_t* status, uint32_t* work, hipStream_t s);
hipError_t launch_staged_flush(const uint32_t* actions, uint32_t* len, uint32_t* head, uint32_t* lost, uint32_t n_peers,
                               hipStream_t s);

}  // namespace wgcs
