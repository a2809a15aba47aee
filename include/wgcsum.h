/*
 * wgcsum.h -- C ABI of the MI355X-native (gfx950) Internet-checksum hot path
 * of muhtutorials/wireguard's `tun` package.
 *
 * Plain C types only (pointers and sizes); no torch, no HIP types in the
 * signatures (streams are passed as `void*` = hipStream_t, NULL = the
 * context's own stream, a blocking stream: ordered both ways with work on the
 * HIP null stream, e.g. torch's default stream).  Every entry point is thread-safe: calls on one
 * context are serialized by a context mutex (the reference serializes Read
 * with Tun.readMu and Write with Tun.writeMu, tun/tun.go:101,:105).
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   wgcs_checksum_batch       batch form of checksum()            tun/checksum.go:152-167
 *                             + checksumValid()                   tun/gro.go:554-612
 *                             + gsoSplit's per-segment L4 sum      tun/gro.go:1469-1488
 *                             + gsoNoneChecksum()                 tun/gro.go:1497-1517
 *                             + IPv4 header checksum sites        tun/gro.go:1134-1138,1217-1221,1434-1436
 *   wgcs_checksum_batches     many such batches enqueued by one call over several streams
 *                             (consecutive Tun.Read / Tun.Write batches, tun/tun.go:477-508, :654-700)
 *   wgcs_checksum             checksum(b, initial)                tun/checksum.go:152-167
 *   wgcs_checksum_valid       checksumValid(pkt, iphLen, proto, isV6)  tun/gro.go:554-612
 *   wgcs_gso_none_checksum    gsoNoneChecksum(readBuf, start, off)     tun/gro.go:1497-1517
 *   wgcs_gso_split            gsoSplit(readBuf, hdr, bufs, sizes, offset, isV6)  tun/gro.go:1373-1493
 *   wgcs_gso_split_batch      device-resident batch of gsoSplit calls  (one per Tun.Read)
 *   wgcs_handle_virtio_read   handleVirtioRead(readBuf, bufs, sizes, offset)  tun/tun.go:514-632
 *   wgcs_*_cap                the same two with cap(readBuf)  (spare capacity, gro.go:1471-1477)
 *   wgcs_handle_gro           handleGRO(bufs, offset, tcpTable, udpTable, canUDPGRO, &toWrite)
 *                                                                 tun/gro.go:1326-1367
 *   wgcs_handle_gro_batch     device-resident batch of handleGRO calls (one per Tun.Write)
 *   wgcs_get_gso_size         getGSOSize(control)                 conn/gso.go:35-67
 *   wgcs_set_gso_size         setGSOSize(&control, gsoSize)       conn/gso.go:71-100
 *   wgcs_split_messages       splitMessages(msgs, firstMsgAt)     conn/bind.go:542-597
 *   wgcs_split_messages_batch device-resident batch of splitMessages calls (one per recvmmsg)
 *   wgcs_coalesce_messages    coalesceMessages(msgs, bufs, ep, addr)  conn/bind.go:599-662
 *   wgcs_coalesce_messages_batch  device-resident batch of coalesceMessages calls (one per Send)
 *   wgcs_aead_*               transport-message Seal / Open       device/send.go:438-463, device/receive.go:363-383
 *   wgcs_router_*             Router (allowed-IPs trie)           device/router.go:405-495
 *   wgcs_session_table_build  SessionMap.Get as an array          device/sessions.go:26-30
 *   wgcs_recv_classify_batch  the loop body of RoutineReceiveFromPeers   device/receive.go:145-207
 *   wgcs_recv_source_batch    the allowed-source check            device/receive.go:438-482
 *   wgcs_route_dst_batch      the routing step of RoutineReadFromTUN     device/send.go:264-293
 *   wgcs_replay_batch         keypair.replayFilter.Validate       device/receive.go:414-420
 *   wgcs_send_assign_batch    keypair.sendNonce and its limit     device/send.go:383-390
 *   wgcs_cookie_*             CookieChecker / CookieGenerator      device/cookie.go
 *   wgcs_handshake_screen_batch  CheckMAC1, CheckMAC2 and the cookie reply at the top of
 *                             RoutineHandshake                     device/receive.go:270-287
 *   wgcs_ratelimit_*          RateLimiter.Allow and cleanup between the screen and the Noise
 *                             code of RoutineHandshake              ratelimiter/ratelimiter.go, device/receive.go:283-286
 *   wgcs_x25519 / _batch      curve25519.X25519                    device/noise_helpers.go:93-105
 *   wgcs_noise_* / wgcs_peer_keys_*  the stateless parts of the Noise handshake's two messages
 *                                                                  device/noise.go:344-457, :494-655
 *   wgcs_handshake_consume_batch  ConsumeMessageInitiation up to its replay / flood check
 *                                                                  device/noise.go:405-457
 *   wgcs_handshake_respond_batch  CreateMessageResponse, AddMACs and the responder's session keys
 *                                                                  device/send.go:130-169
 *   wgcs_write_build_batch    one Tun.Write per receive batch and peer, with the peer's
 *                             bookkeeping (_host: on host arrays) device/receive.go:178-228, :398-504
 *   wgcs_timers_*             the peer timers, their event hooks and their expiry  device/timers.go
 *   wgcs_staged_*             peer.qus.staged: StagePackets, SendStagedPackets, FlushStagedPackets
 *                                                                  device/send.go:331-426
 *   wgcs_stager_*            Tun.Read batch staging              tun/tun.go:477-508
 *   wgcs_wstager_*            Tun.Write batch staging             tun/tun.go:654-700
 * Status codes map 1:1 onto the reference's Go errors (see WGCS_ERR_*).
 */
#ifndef WGCSUM_H
#define WGCSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGCS_ABI_VERSION 2 /* 2: wgcs_pkt carries proto and a u16 csum_offset */

/* ---- status codes (negative); Go sentinel / error each one maps to ---- */
#define WGCS_OK 0
#define WGCS_ERR_INVALID_ARG (-1)       /* API misuse (NULL ctx, n too large, ...) */
#define WGCS_ERR_SHORT_BUFFER (-2)      /* io.ErrShortBuffer                 gro.go:75,86 */
#define WGCS_ERR_TOO_MANY_SEGMENTS (-3) /* tun.ErrTooManySegments            tun.go:30, gro.go:1410 */
#define WGCS_ERR_INVALID_OFFSET (-4)    /* errors.New("invalid offset")     gro.go:1336 */
#define WGCS_ERR_UNSUPPORTED_GSO (-5)   /* "unsupported virtio GSO type: %d" tun.go:567 */
#define WGCS_ERR_IP_GSO_MISMATCH (-6)   /* "IP header version: %d, GSO type: %d" tun.go:575,584 */
#define WGCS_ERR_BAD_IP_VERSION (-7)    /* "invalid IP header version: %d"  tun.go:591 */
#define WGCS_ERR_PACKET_TOO_SHORT (-8)  /* "packet is too short"            tun.go:603 */
#define WGCS_ERR_TCP_HDR_LEN (-9)       /* "TCP header length is invalid: %d" tun.go:611 */
#define WGCS_ERR_HDR_LEN (-10)          /* "length of packet (%d) < virtioNetHdr.hdrLen (%d)" tun.go:616 */
#define WGCS_ERR_CSUM_OFFSET (-11)      /* "end of checksum offset (%d) exceeds packet length (%d)" tun.go:625 */
#define WGCS_ERR_READ_OVERFLOW (-12)    /* "read length %d overflows bufs element length %d" tun.go:546 */
#define WGCS_ERR_OUT_OF_RANGE (-13)     /* input on which the Go code would panic (slice bounds) */
#define WGCS_ERR_BATCH_FULL (-14)       /* stager: the open batch has no room; submit it first.
                                           wgcs_write_build_batch: a batch has more peers than calls_per_batch */
#define WGCS_ERR_NOT_READY (-15)        /* stager: batch id not submitted / recycled */
#define WGCS_ERR_CMSG (-16)             /* "error parsing socket control message: %w" conn/gso.go:45 */
#define WGCS_ERR_SPLIT_OVERFLOW (-17)   /* "splitting coalesced packet resulted in overflow" conn/bind.go:565 */
#define WGCS_ERR_AUTH (-18)             /* "chacha20poly1305: message authentication failed" receive.go:380 */
#define WGCS_ERR_SOURCE (-19)           /* "packet with disallowed source address" receive.go:452-457, :472-477 */
#define WGCS_ERR_REPLAY (-20)           /* replayFilter.Validate said no: the packet is dropped  receive.go:418-420 */
#define WGCS_ERR_MAC1 (-21)             /* "Received packet with invalid mac1" receive.go:272-275 */
#define WGCS_ERR_LOW_ORDER (-22)        /* "bad input point: low order point" curve25519.X25519, noise.go:421-424 */
#define WGCS_ERR_NO_PEER (-23)          /* GetPeer found none, or it is not running / has no shared secret  noise.go:432-443 */
#define WGCS_ERR_NO_HANDSHAKE (-24)    /* sessions.Get(msg.Receiver) finds no handshake, or its state is not
                                          handshakeInitiationCreated  noise.go:553-557, :566 */
#define WGCS_ERR_HIP (-100)          /* HIP runtime error (message: wgcs_last_error) */
#define WGCS_ERR_NOMEM (-101)
#define WGCS_ERR_NO_DEVICE (-102)

/* ---- batch descriptor: one packet (or byte range) in a device arena ----
 * 16 bytes, loaded by the kernels as one dwordx4.  The arena offset is 48 bits
 * (off_lo | off_hi << 32); the checksum field sits at the uint16 position
 * (csum_start + csum_offset) & 0xFFFF, as the reference computes it
 * (gro.go:1391, :1503).  wgcs_pkt_set() fills one. */
typedef struct wgcs_pkt {
  uint32_t off_lo;      /* byte offset of the packet (IP header) in the arena, bits 0-31 */
  uint16_t off_hi;      /* bits 32-47                                                    */
  uint8_t proto;        /* pseudo-header protocol (checksumValid's `protocol`, any u8)   */
  uint8_t flags;        /* WGCS_PKT_*                                                    */
  uint32_t len;         /* packet length in bytes (< 2^31)                               */
  uint16_t csum_start;  /* L4 start = IP header length (iphLen / virtio csumStart)       */
  uint16_t csum_offset; /* checksum field offset from csum_start (16 TCP, 6 UDP, any)    */
} wgcs_pkt;

#define WGCS_PKT_V6 0x01 /* isV6: addresses at 8/24 (16 B) instead of 12/16 (4 B) */

static inline void wgcs_pkt_set(wgcs_pkt *p, uint64_t off, uint32_t len, uint16_t csum_start,
                                uint16_t csum_offset, uint8_t proto, uint8_t flags) {
  p->off_lo = (uint32_t)off;
  p->off_hi = (uint16_t)(off >> 32);
  p->proto = proto;
  p->flags = flags;
  p->len = len;
  p->csum_start = csum_start;
  p->csum_offset = csum_offset;
}

/* ---- batch modes (out element: u16, except VALIDATE: u8 0/1) ---- */
#define WGCS_MODE_FOLD 0     /* out = checksum(pkt[0:len], initial[i])                 checksum.go:152 */
#define WGCS_MODE_L4_FILL 1  /* out = ^checksum(pkt[cs:len] with field zeroed,
                                pseudoHeaderChecksumNoFold(src,dst,proto,len-cs))     gro.go:1469-1488 */
#define WGCS_MODE_VALIDATE 2 /* out = checksumValid(pkt, cs, proto, isV6)             gro.go:554-612 */
#define WGCS_MODE_PARTIAL 3  /* out = ^checksum(pkt[cs:len] field zeroed, BE16(field)) gro.go:1497-1517 */
#define WGCS_MODE_IP4HDR 4   /* out = ^checksum(pkt[0:cs] with [10:12] zeroed, 0)      gro.go:1134-1138 */

#define WGCS_F_INPLACE 0x1 /* also store the result big-endian into the packet's field
                              (when the field lies inside the packet's len bytes) */

typedef struct wgcs_ctx wgcs_ctx;

/* virtioNetHdr, tun/gro.go:42-67 (10 bytes on the wire, native byte order) */
typedef struct wgcs_virtio_hdr {
  uint8_t flags;
  uint8_t gso_type;
  uint16_t hdr_len;
  uint16_t gso_size;
  uint16_t csum_start;
  uint16_t csum_offset;
} wgcs_virtio_hdr;

/* one job of wgcs_gso_split_batch: a Tun.Read super-packet */
typedef struct wgcs_gso_job {
  uint64_t off;   /* offset of the 10-byte virtio header in the device arena */
  uint32_t len;   /* bytes read from the TUN fd (virtio header included)     */
  uint32_t flags; /* WGCS_GSO_JOB_*                                          */
} wgcs_gso_job;

/* default (0): handleVirtioRead semantics -- validate the header, recompute
 * hdrLen, GSO_NONE copy (+ gsoNoneChecksum), tun/tun.go:514-632.
 * RAW: gsoSplit(readBuf, hdr, ...) semantics with the header fields taken as
 * given (gro.go:1373-1493); WGCS_GSO_JOB_V6 then gives isV6. */
#define WGCS_GSO_JOB_RAW 0x1u
#define WGCS_GSO_JOB_V6 0x2u
/* bits 8-15: how many bytes after the job's len bytes in the arena belong to
 * the read buffer's spare capacity (cap(readBuf) - len(readBuf), at most 255).
 * The pseudo-header address slices of a packet shorter than 20 / 40 bytes
 * reach into it (gro.go:1471-1477: a slice up to cap is legal Go); past it
 * the reference panics (OUT_OF_RANGE).  0: cap == len. */
#define WGCS_GSO_JOB_SPARE(n) ((uint32_t)((n) > 255 ? 255 : (n)) << 8)

/* ---- lifecycle / diagnostics ---- */
int wgcs_abi_version(void);
int wgcs_device_count(int *count);
int wgcs_init(int device, wgcs_ctx **out);
/* INVALID_ARG (the context stays usable) while a read or write stager made
 * on it is alive: destroy the stagers first. */
int wgcs_destroy(wgcs_ctx *ctx);
const char *wgcs_strerror(int status);
/* The calling thread's last error message on ctx (like errno: per thread, so
 * concurrent callers never share one buffer); "" when this thread's last
 * failure was on another context.  Valid until the thread's next failing call. */
const char *wgcs_last_error(wgcs_ctx *ctx);
int wgcs_sync(wgcs_ctx *ctx);
/* CU count of the context's device (grid sizing, reporting) */
int wgcs_num_cu(wgcs_ctx *ctx);
/* Pinned host memory mapped into the device's address space at the same
 * address (bytes rounded up to 16): the buffers of wgcs_wstager_push_pinned. */
int wgcs_host_alloc(wgcs_ctx *ctx, size_t bytes, void **p);
/* NOT_READY while a write-stager slot still reads the allocation (a recorded
 * zero-copy push, open or in flight); safe against concurrent
 * wgcs_wstager_push_pinned calls: either the push is refused (INVALID_ARG) or
 * the free is (NOT_READY). */
int wgcs_host_free(wgcs_ctx *ctx, void *p);

/* ---- device-resident batch entry points (HBM in, HBM out; async on stream) ----
 * The arena must be readable through align_up(off+len, 16) for every packet
 * (always true for hipMalloc / torch allocations, which are page-granular).
 * VALIDATE / L4_FILL read the pseudo-header addresses at [12, 20) / [8, 40)
 * whatever len is: a packet shorter than them has them read from the arena
 * bytes after it, its Go slice's spare capacity (gro.go:558-563), which must
 * then be readable too.  A csum_start past len (pkt[iphLen:] panics in Go)
 * gives VALIDATE 0 and L4_FILL 0 with no field write. */
int wgcs_checksum_batch(wgcs_ctx *ctx, int mode, unsigned flags, uint8_t *d_arena,
                        const wgcs_pkt *d_pkts, const uint64_t *d_initial, uint32_t n,
                        void *d_out, void *stream);

/* A series of independent device-resident batches enqueued by one call (e.g.
 * consecutive Tun.Read/Write batches, tun/tun.go:477-508, :654-700, already in
 * HBM), each with wgcs_checksum_batch's semantics.  The list is dealt over
 * streams[0 .. n_streams) (n_streams 0: the context's stream): batch k belongs
 * to streams[k % n_streams].
 *
 * Promised:
 *  - ordering against each listed stream's other work: batch k starts after
 *    everything queued earlier on its stream (a copy that fills its arena),
 *    and whatever is queued later on a listed stream that has a batch, or a
 *    wait on such a stream, comes after EVERY batch of the call -- all results
 *    are ready when any one of those streams is;
 *  - with WGCS_F_INPLACE, batches k and k + n_streams run in list order (they
 *    share a stream), as do all batches on one stream;
 *  - two batches whose `out` ranges overlap without being the same (arena,
 *    pkts, initial, out, n) tuple leave the later batch's results there;
 *  - every batch of the list is read and summed in full, repeated ones too;
 *  - optional bracket events (hipEvent_t as void*, created by the caller):
 *    ev_begin is recorded on streams[0] before the first launch and ev_end on
 *    streams[0] after the last, so the pair spans every launch.
 * Not promised: that batch k physically runs on streams[k % n_streams], or any
 * order between the batches of one call without WGCS_F_INPLACE.  Consecutive
 * batches that may run concurrently are processed by one launch on streams[0]
 * (up to 32 per launch, walking the batches in list order; the other listed
 * streams are joined before it and forked after it).  WGCS_F_INPLACE, or the
 * diagnostic switch WGCS_FUSE=0 in the environment at wgcs_init, keeps one
 * launch per batch on streams[k % n_streams]: a listed stream's later work
 * then follows that stream's own batches only, and ev_end, or a wait on every
 * listed stream, covers them all.
 * All arguments are checked before anything is enqueued. */
typedef struct wgcs_batch {
  uint8_t *arena;
  const wgcs_pkt *pkts;
  const uint64_t *initial; /* FOLD only; may be NULL */
  void *out;
  uint32_t n;
  uint32_t pad;
} wgcs_batch;
#define WGCS_MAX_BATCH_STREAMS 16
int wgcs_checksum_batches(wgcs_ctx *ctx, int mode, unsigned flags, const wgcs_batch *batches,
                          uint32_t n_batches, void *const *streams, uint32_t n_streams,
                          void *ev_begin, void *ev_end);

/* A doorbell: work enqueued on `stream` (NULL: the context's) after this call
 * starts only once *flag == value.  `flag` is a 4-byte-aligned word of
 * wgcs_host_alloc memory (the device polls it); the host rings it with a plain
 * store.  A receive / send ring posts its batches ahead of time and rings once
 * they are due, so no host enqueue cost sits between a batch being ready and
 * its launch.  The caller must ring before it waits on the stream. */
int wgcs_stream_wait_flag(wgcs_ctx *ctx, void *stream, const uint32_t *flag, uint32_t value);

/* gsoSplit for n_jobs super-packets.  Job j writes its segments into output
 * slots [j*max_segs, (j+1)*max_segs), slot s at d_out + s*out_stride + offset
 * (like bufs[s][offset:]).  d_sizes[slot] = packet size; d_count[j] = the
 * return value n (>= 0) and d_status[j] = 0 or a WGCS_ERR_* code, with the
 * reference's ErrTooManySegments semantics (n = max_segs-1, gro.go:1409-1410).
 * d_sizes is written for the slots the job reaches only (d_count[j] of them;
 * all max_segs with TOO_MANY_SEGMENTS); the other rows and slots keep what
 * they held.
 * Includes handleVirtioRead's GSO validation (tun/tun.go:557-631).
 * INVALID_ARG for max_segs == 0, max_segs >= 2^31 (len(bufs) is a Go int) or
 * n_jobs * max_segs >= 2^32. */
int wgcs_gso_split_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_gso_job *d_jobs,
                         uint32_t n_jobs, uint8_t *d_out, uint32_t out_stride, uint32_t offset,
                         uint32_t max_segs, int32_t *d_sizes, int32_t *d_count,
                         int32_t *d_status, void *stream);
/* the shape wgcs_gso_split_batch was compiled to (not a reference interface:
 * benches and profiles name the kernel from it): lds_waves waves per
 * workgroup, parts workgroups per read, u chunks per lane in flight; rows = 1
 * when WGCS_GSO_KERNEL=rows selects the round-4 gso_rows_kernel grid. */
int wgcs_gso_kernel_shape(int *lds_waves, int *parts, int *u, int *rows);

/* ---- reference-shaped entry points on host buffers (Go-call granularity) ----
 * These stage through the context's pinned ring, run the HIP kernels and copy
 * results back; they keep the reference's argument meaning and errors. */
int wgcs_checksum(wgcs_ctx *ctx, const uint8_t *b, size_t n, uint64_t initial, uint16_t *out);
int wgcs_checksum_valid(wgcs_ctx *ctx, const uint8_t *pkt, size_t len, uint8_t iph_len,
                        uint8_t proto, int is_v6, int *valid);
/* the same with the slice's capacity: pkt[0, cap) is readable, and a packet
 * shorter than its addresses (20 / 40 B) has them read from pkt[len, cap), as
 * Go's pkt[a:b] up to cap does (gro.go:558-563); OUT_OF_RANGE past cap or for
 * iph_len > len.  wgcs_checksum_valid is this with cap == len. */
int wgcs_checksum_valid_cap(wgcs_ctx *ctx, const uint8_t *pkt, size_t len, size_t cap,
                            uint8_t iph_len, uint8_t proto, int is_v6, int *valid);
int wgcs_gso_none_checksum(wgcs_ctx *ctx, uint8_t *read_buf, size_t len, uint16_t csum_start,
                           uint16_t csum_offset);
/* host batch: same semantics as wgcs_checksum_batch on a host arena of
 * arena_len bytes; VALIDATE / L4_FILL packets whose pseudo-header addresses
 * would lie past it are refused (OUT_OF_RANGE: the arena is their capacity) */
int wgcs_checksum_batch_host(wgcs_ctx *ctx, int mode, unsigned flags, uint8_t *h_arena,
                             size_t arena_len, const wgcs_pkt *h_pkts, const uint64_t *h_initial,
                             uint32_t n, void *h_out);
/* bufs[i] points at a buffer of buf_lens[i] bytes; sizes[] receives packet sizes. */
int wgcs_gso_split(wgcs_ctx *ctx, uint8_t *read_buf, size_t len, const wgcs_virtio_hdr *hdr,
                   uint8_t *const *bufs, const size_t *buf_lens, int nbufs, int *sizes,
                   int offset, int is_v6, int *n_out);
/* read_buf: the bytes read from the TUN fd, virtio header first (tun/tun.go:490). */
int wgcs_handle_virtio_read(wgcs_ctx *ctx, uint8_t *read_buf, size_t n, uint8_t *const *bufs,
                            const size_t *buf_lens, int nbufs, int *sizes, int offset,
                            int *n_out);
/* The same with the slice's capacity: read_buf[0, cap) is readable and
 * read_buf[n, cap) is the spare capacity Tun.Read's tun.readBuf[:n] carries
 * (tun/tun.go:484-503); only the pseudo-header address slices of a packet
 * shorter than its IP addresses reach it (gro.go:1471-1477).  cap >= n;
 * wgcs_handle_virtio_read is this with cap == n.  Same for gsoSplit. */
int wgcs_handle_virtio_read_cap(wgcs_ctx *ctx, uint8_t *read_buf, size_t n, size_t cap,
                                uint8_t *const *bufs, const size_t *buf_lens, int nbufs,
                                int *sizes, int offset, int *n_out);
int wgcs_gso_split_cap(wgcs_ctx *ctx, uint8_t *read_buf, size_t len, size_t cap,
                       const wgcs_virtio_hdr *hdr, uint8_t *const *bufs, const size_t *buf_lens,
                       int nbufs, int *sizes, int offset, int is_v6, int *n_out);
/* Go-slice form of handleGRO: lens[i] = len(bufs[i]), caps[i] = cap(bufs[i]).
 * bufs/lens/caps are updated in place (appends grow lens[i]; prepends swap
 * entries, gro.go:696-697); to_write receives the indices to write. */
int wgcs_handle_gro(wgcs_ctx *ctx, uint8_t **bufs, size_t *lens, size_t *caps, int n,
                    int offset, int can_udp_gro, int *to_write, int *n_to_write);

/* ---- the resident per-call ring (round 6) ----
 * The per-call forms above pay one kernel launch plus one completion wait per
 * Go call (~20 us).  A ring keeps a small kernel resident on a few CUs of its
 * own stream: a call writes a request record in fine-grained pinned host
 * memory and spins on a completion word the kernel bumps, so one Tun.Read /
 * checksumValid costs a PCIe round trip instead of a launch.  Same arguments,
 * bytes and errors as wgcs_checksum_valid[_cap] / wgcs_handle_virtio_read[_cap]
 * (tun/gro.go:554-612, tun/tun.go:514-632).  Request bytes in wgcs_host_alloc
 * memory are read in place; other caller memory is copied into the ring's
 * staging.  The kernel leaves after idle_us (0: 100 ms) without a request and
 * a later call launches it again; one call at a time per ring (it locks).
 * wgcs_ring_destroy stops the kernel and waits for it. */
typedef struct wgcs_ring wgcs_ring;
int wgcs_ring_create(wgcs_ctx *ctx, uint32_t idle_us, wgcs_ring **out);
int wgcs_ring_destroy(wgcs_ring *ring);
/* requests served, kernel launches made, 1 while the kernel is resident */
int wgcs_ring_info(wgcs_ring *ring, uint64_t *requests, uint64_t *launches, int *running);
int wgcs_ring_checksum_valid(wgcs_ring *ring, const uint8_t *pkt, size_t len, uint8_t iph_len, uint8_t proto,
                             int is_v6, int *valid);
int wgcs_ring_checksum_valid_cap(wgcs_ring *ring, const uint8_t *pkt, size_t len, size_t cap, uint8_t iph_len,
                                 uint8_t proto, int is_v6, int *valid);
int wgcs_ring_handle_virtio_read(wgcs_ring *ring, uint8_t *read_buf, size_t n, uint8_t *const *bufs,
                                 const size_t *buf_lens, int nbufs, int *sizes, int offset, int *n_out);
int wgcs_ring_handle_virtio_read_cap(wgcs_ring *ring, uint8_t *read_buf, size_t n, size_t cap,
                                     uint8_t *const *bufs, const size_t *buf_lens, int nbufs, int *sizes,
                                     int offset, int *n_out);

/* ---- device-resident batch of Tun.Write calls (handleGRO per call) ----
 * bufs[i] of a call is the Go slice d_arena[off : off+len] with cap(bufs[i]) =
 * cap; every slice owns d_arena[off, off+cap), and the arena must be readable
 * through align_up(off+cap, 16).  Call c runs handleGRO(bufs[first :
 * first+n], offset, ..., canUDPGRO = flags & WGCS_GRO_CAN_UDP) on the device,
 * in place, as the reference mutates its slices: the slice headers in d_bufs
 * after the prepend swaps and appends (gro.go:685-697), d_status[c] = 0,
 * WGCS_ERR_INVALID_OFFSET (gro.go:1335-1337: the earlier buffers keep what the
 * coalescing wrote, nothing is applied, d_n_write[c] = 0) or
 * WGCS_ERR_INVALID_ARG (n > WGCS_GRO_MAX_CALL or offset < 0: nothing touched),
 * and toWrite in d_to_write[first : first + d_n_write[c]].  Every byte that
 * Tun.Write hands to write(2) -- bufs[i][offset-10:len] for i in toWrite --
 * equals the reference's, and so does every other byte of every slice.
 * A call with n == 0 is a no-op: d_status[c] = 0, d_n_write[c] = 0, and nothing
 * else is read or written -- not d_bufs, not d_to_write, not the arena.  The
 * fixed layout of wgcs_write_build_batch relies on it: its unused call rows
 * and the calls of peers without a packet to write are such calls.
 * One workgroup per call, async on stream. */
typedef struct wgcs_gro_buf {
  uint64_t off; /* slice start in the arena */
  uint32_t len; /* len(bufs[i]) (offset + packet length) */
  uint32_t cap; /* cap(bufs[i]) */
} wgcs_gro_buf;
typedef struct wgcs_gro_call {
  uint32_t first; /* index of bufs[0] in d_bufs (and of toWrite[0] in d_to_write) */
  uint32_t n;     /* len(bufs) */
  int32_t offset; /* Tun.Write's offset */
  uint32_t flags; /* WGCS_GRO_CAN_UDP */
} wgcs_gro_call;
#define WGCS_GRO_CAN_UDP 0x1u
#define WGCS_GRO_MAX_CALL 128 /* conn.BatchSize (conn/conn.go:14): the largest Write batch */
int wgcs_handle_gro_batch(wgcs_ctx *ctx, uint8_t *d_arena, wgcs_gro_buf *d_bufs, const wgcs_gro_call *d_calls,
                          uint32_t n_calls, int32_t *d_status, int32_t *d_n_write, int32_t *d_to_write,
                          void *stream);

/* ---- Tun.Read batch staging (tun/tun.go:477-508) ----
 * A ring of `depth` batches.  Each batch stages up to max_reads TUN reads
 * (virtio header + packet, as read(2) returns them into tun.readBuf) in pinned
 * host memory; wgcs_stager_submit queues H2D -> GSO split (the kernel of
 * wgcs_gso_split_batch, handleVirtioRead semantics) -> D2H of sizes, counts,
 * statuses and the output slots on the batch's own stream, so consecutive
 * batches overlap both copy directions with compute.  Segment s of read r
 * lands in pinned memory at segs + s*seg_stride (seg_stride >= the largest
 * segment, e.g. 65535 for 64 KiB GSO_NONE reads, 1536 for MSS 1460).
 * Only the stager's own copy of each read is used (tun.readBuf is free again
 * as soon as push/commit returns); the reference's in-place readBuf edits are
 * not replayed there (they are invisible to Read's callers).
 * Ring discipline (depth >= 2): one slot is always open for pushes, so the results of a
 * batch stay readable until depth-1 further batches have been submitted
 * (the submit after that recycles its slot, waiting for it if still running). */
typedef struct wgcs_stager wgcs_stager;
int wgcs_stager_create(wgcs_ctx *ctx, uint32_t depth, uint32_t max_reads, size_t max_bytes,
                       uint32_t max_segs, uint32_t seg_stride, wgcs_stager **out);
int wgcs_stager_destroy(wgcs_stager *st);
/* copy one read into the open batch (waits for the ring slot if it is still in flight) */
int wgcs_stager_push(wgcs_stager *st, const uint8_t *read_buf, size_t n, int *read_idx);
/* push `count` reads in one call (read_idx of the first one in *first_idx); on
 * WGCS_ERR_BATCH_FULL *pushed tells how many went in */
int wgcs_stager_push_many(wgcs_stager *st, const uint8_t *const *read_bufs, const size_t *ns, int count,
                          int *first_idx, int *pushed);
/* zero-copy form: reserve room for up to max_n bytes (read(2) goes straight
 * into *dst), then commit the byte count read (0 drops the reservation).  If
 * the read's output region does not fit the open batch, commit returns
 * WGCS_ERR_BATCH_FULL and keeps the bytes: the next wgcs_stager_submit queues
 * the batch without them and carries them in as read 0 of the new batch. */
int wgcs_stager_reserve(wgcs_stager *st, size_t max_n, uint8_t **dst, int *read_idx);
int wgcs_stager_commit(wgcs_stager *st, int read_idx, size_t n);
/* queue the open batch (no-op id for an empty batch) and open the next one */
int wgcs_stager_submit(wgcs_stager *st, uint64_t *batch);
int wgcs_stager_wait(wgcs_stager *st, uint64_t batch);
/* results of read r of a completed batch, handleVirtioRead's (n, err) */
int wgcs_stager_result(wgcs_stager *st, uint64_t batch, int read_idx, int *status, int *n,
                       const int32_t **sizes, const uint8_t **segs);
/* copy read r's segments into bufs[i][offset:] exactly as handleVirtioRead
 * leaves them (sizes[], n, ErrTooManySegments / slice-bound checks).  `segs`
 * of wgcs_stager_result holds the packets only: for a read whose header
 * geometry writes past a segment's end or reads bufs[i][4:6] (an IPv4 header
 * shorter than 6 bytes), copy_out runs the read again through the per-call
 * path with these bufs, so that every byte matches (gro.go:1419-1488).  That
 * rerun is a synchronous GPU round trip under the context's lock; it runs on a
 * copy of the read with the stager unlocked, so other calls on the stager do
 * not wait for it. */
int wgcs_stager_copy_out(wgcs_stager *st, uint64_t batch, int read_idx, uint8_t *const *bufs,
                         const size_t *buf_lens, int nbufs, int *sizes, int offset, int *n_out);

/* ---- Tun.Write batch staging (tun/tun.go:654-700) ----
 * A ring of `depth` slots; a slot aggregates up to max_writes Tun.Write calls
 * (<= max_pkts packets and <= max_bytes packet bytes in all).
 * wgcs_wstager_push stages one Write call (n <= WGCS_GRO_MAX_CALL buffers) --
 * bufs[i][offset-10:lens[i]], the packets as device/receive.go:483 slices
 * them, caps[i] = cap(bufs[i]) -- into pinned memory; no host planning.
 * wgcs_wstager_submit queues, on the slot's own stream, one H2D of every staged
 * packet, ONE device-resident handleGRO launch over every staged call (the
 * kernel of wgcs_handle_gro_batch: flow tables, checksumValid, coalescing and
 * apply* per call, on Go-sized slices in HBM), a gather of every call's
 * toWrite images and one D2H, so results are exactly handleGRO's
 * (gro.go:1326-1367).  wgcs_wstager_wait waits for the slot.
 * wgcs_wstager_result hands back, per call, what
 * Tun.Write passes to write(2) (tun.go:687-698): to_write[k] = handleGRO's
 * toWrite and pkts[k][0:pkt_lens[k]] = bufs[to_write[k]][offset-10:] after
 * handleGRO (10-byte virtio header + packet) in pinned memory, valid until the
 * slot is recycled; status WGCS_ERR_INVALID_OFFSET (gro.go:1336) writes
 * nothing.  The caller's bufs are only read.  Ring discipline as the Read
 * stager's: results stay readable until depth-1 more submits. */
typedef struct wgcs_wstager wgcs_wstager;
int wgcs_wstager_create(wgcs_ctx *ctx, uint32_t depth, uint32_t max_writes, uint32_t max_pkts, size_t max_bytes,
                        wgcs_wstager **out);
int wgcs_wstager_destroy(wgcs_wstager *ws);
/* stage one Tun.Write(bufs, offset) call; *write_idx = its index in the open slot
 * (WGCS_ERR_BATCH_FULL: submit first) */
int wgcs_wstager_push(wgcs_wstager *ws, const uint8_t *const *bufs, const size_t *lens, const size_t *caps, int n,
                      int offset, int can_udp_gro, int *write_idx);
/* Zero-copy form: every bufs[i] lies in memory from wgcs_host_alloc and stays
 * unchanged until the slot's results have been read; push records descriptors
 * only and the slot's scatter kernel reads the packets from host memory over
 * PCIe (a buffer pool allocated this way, e.g. device.pools.messageBufs, lets
 * Write skip the staging copy). */
int wgcs_wstager_push_pinned(wgcs_wstager *ws, const uint8_t *const *bufs, const size_t *lens, const size_t *caps,
                             int n, int offset, int can_udp_gro, int *write_idx);
int wgcs_wstager_submit(wgcs_wstager *ws, uint64_t *batch);
int wgcs_wstager_wait(wgcs_wstager *ws, uint64_t batch);
/* to_write / pkts / pkt_lens hold at least n (the call's packet count) entries */
int wgcs_wstager_result(wgcs_wstager *ws, uint64_t batch, int write_idx, int *status, int *n_write, int *to_write,
                        const uint8_t **pkts, size_t *pkt_lens);

/* ---- outer-UDP message batching (conn/bind.go, conn/gso.go) ----
 * The UDP side of the same batch loop: recvmmsg with UDP_GRO hands back up to
 * BatchSize/64 coalesced datagrams that splitMessages cuts into packets, and
 * Send coalesces runs of equal-size packets for UDP_SEGMENT (conn/bind.go:25-36:
 * maxIPv4PayloadLen 65507, maxIPv6PayloadLen 65527, maxUDPSegments 64). */

/* getGSOSize(msg.OOB[:msg.NN]): the UDP_GRO size (0 if absent) or WGCS_ERR_CMSG */
int wgcs_get_gso_size(const uint8_t *control, size_t len, int *gso_size);
/* setGSOSize(&control, gsoSize): appends a SOL_UDP/UDP_SEGMENT cmsg (24 bytes)
 * when it fits in cap; *len is len(control) in and out */
int wgcs_set_gso_size(uint8_t *control, size_t *len, size_t cap, uint16_t gso_size);

/* splitMessages over n_batches recvmmsg batches of n_msgs messages each.
 * At most 128 source messages (n_msgs - first_msg_at <= 128; BatchSize is 128,
 * conn/conn.go:14).  Message slot q = b*n_msgs + s.  Input: the recvmmsg landing buffers only --
 * msgs[s].Buffers[0] for s >= first_msg_at (buf_len bytes, len == cap) at
 * d_in + (b*(n_msgs - first_msg_at) + s - first_msg_at)*in_stride;
 * d_n_in[q] = msgs[s].N (all s), d_gso[q] = getGSOSize result (>= 0) or WGCS_ERR_CMSG.
 * Output, out of place: packet k of batch b at d_out + (b*n_msgs + k)*out_stride
 * (16-byte aligned, out_stride >= the largest packet), d_n_out[q] = the final
 * msgs[s].N (packet length, 0 for a source zeroed by :589-594, else unchanged),
 * d_src[q] = index s' whose Addr the slot now carries (:570) or -1 if unchanged;
 * d_count[b] = nPackets, d_status[b] = 0 / WGCS_ERR_CMSG / WGCS_ERR_SPLIT_OVERFLOW /
 * WGCS_ERR_OUT_OF_RANGE (Buffers[0][0:gsoSize] beyond cap) / WGCS_ERR_INVALID_ARG
 * (N > buf_len or a packet larger than out_stride).  On an error status the
 * packets before it are written, as the reference copies them before returning.
 * No byte of d_out outside [slot, slot + d_n_out) of the packets below d_count[b]
 * is written: the rest of such a slot and every slot at or past d_count[b] keep
 * what they held (d_n_out there is the d_n_in given: 0 for a pool message and
 * for a source whose packets went elsewhere; d_src is -1).  d_in, d_n_in and
 * d_gso are only read.  So wgcs_recv_classify_batch may run over all
 * n_batches * n_msgs slots with d_n_out as its d_size. */
int wgcs_split_messages_batch(wgcs_ctx *ctx, const uint8_t *d_in, uint64_t in_stride, uint32_t buf_len,
                              const int32_t *d_n_in, const int32_t *d_gso, uint32_t n_msgs,
                              uint32_t first_msg_at, uint32_t n_batches, uint8_t *d_out,
                              uint64_t out_stride, int32_t *d_n_out, int32_t *d_src, int32_t *d_count,
                              int32_t *d_status, void *stream);

/* coalesceMessages over n_batches Send batches, in place.  Batch b has
 * d_nbufs[b] <= max_bufs buffers; buffer j is slot q = b*max_bufs + j at
 * d_bufs + q*buf_stride (16-byte aligned), len(bufs[j]) = d_lens[q],
 * cap(bufs[j]) = min(d_caps[q], buf_cap) (d_caps NULL: buf_cap; buf_cap <= buf_stride).
 * Appends land in the first buffer of each run, as Go's append within cap does.
 * Per batch: d_n_msgs[b] = nMsgs; per message m (index b*max_bufs + m):
 * d_msg_first = the buffer j that msgs[m].Buffers[0] aliases, d_msg_len = its
 * final length, d_msg_gso = the UDP_SEGMENT size set by setGSOSize, or -1 if none.
 * No byte of d_bufs outside [0, cap) of a batch's first d_nbufs[b] buffers is
 * written: what lies between a buffer's capacity and its slot's end, and the
 * slots at or past d_nbufs[b], keep what they held.  d_lens and d_caps are read
 * below d_nbufs[b] only, so the rows past it may hold anything (with
 * wgcs_aead_seal_batch's d_out_len as d_lens: its negative refusals, or rows it
 * never wrote); the message rows at or past d_n_msgs[b] are not written. */
int wgcs_coalesce_messages_batch(wgcs_ctx *ctx, uint8_t *d_bufs, uint64_t buf_stride, uint32_t buf_cap,
                                 const int32_t *d_caps, const int32_t *d_lens, const int32_t *d_nbufs,
                                 uint32_t max_bufs, uint32_t n_batches, int dst_is_v6, int32_t *d_n_msgs,
                                 int32_t *d_msg_first, int32_t *d_msg_len, int32_t *d_msg_gso,
                                 void *stream);

/* splitMessages(msgs, firstMsgAt) on host buffers: bufs[i] = msgs[i].Buffers[0]
 * (buf_len bytes each, len == cap, as device/receive.go:119 passes them),
 * ns[i] = msgs[i].N (in/out), oobs[i][0:nns[i]] = msgs[i].OOB[:msgs[i].NN];
 * addr_src[i] = the message whose Addr msgs[i] carries afterwards (i if unchanged).
 * Returns the status, *n_packets = nPackets. */
int wgcs_split_messages(wgcs_ctx *ctx, uint8_t *const *bufs, size_t buf_len, int *ns,
                        const uint8_t *const *oobs, const size_t *nns, int n_msgs, int first_msg_at,
                        int *addr_src, int *n_packets);
/* coalesceMessages(msgs, bufs, endpoint, addr) on host buffers (len/cap per
 * buffer, len <= 65536): appends into bufs[msg_first[m]] within its capacity;
 * msg_len[m] = len(msgs[m].Buffers[0]).  oobs (optional, m < nbufs): msgs[m].OOB
 * with oob_lens in/out and oob_caps -- setSrcControl(src_ctl) then setGSOSize
 * for runs of > 1 packet, as conn/bind.go:634,647,657 do.  *n_msgs = nMsgs. */
int wgcs_coalesce_messages(wgcs_ctx *ctx, uint8_t *const *bufs, const size_t *lens, const size_t *caps,
                           int nbufs, int dst_is_v6, const uint8_t *src_ctl, size_t src_len,
                           uint8_t *const *oobs, size_t *oob_lens, const size_t *oob_caps,
                           int *msg_first, size_t *msg_len, int *n_msgs);

/* ---- transport AEAD (device/send.go:438-463, device/receive.go:363-383, :432-482)
 * ChaCha20-Poly1305 (RFC 8439) with empty additional data and the nonce
 * 4 zero bytes | LE64 counter, on transport messages
 *   LE32 type 4 | LE32 receiver index | LE64 counter | ciphertext | 16-byte tag.
 * Batches work in place on packets at any byte offset of one arena. */

/* One session key in device memory (4-byte aligned).  The table is the
 * caller's: clear or overwrite it on rekey. */
typedef struct wgcs_aead_key {
  uint8_t key[32];
  uint32_t remote_index; /* SEAL: the receiver index written into the header */
  uint32_t pad[3];
} wgcs_aead_key; /* 48 B */

/* One packet: SEAL  plaintext of len bytes at off + 16, sealed under
 *                   (keys[key], counter); room for the header before it and
 *                   for padding and tag after it;
 *             OPEN  the whole transport message of len bytes at off (counter
 *                   is not read: it comes from message bytes [8, 16)). */
typedef struct wgcs_aead_pkt {
  uint64_t off;
  uint64_t counter;
  uint32_t len;
  uint32_t key;
} wgcs_aead_pkt; /* 24 B, 8-byte aligned */

/* padding(packetSize, mtu) of send.go:529-560 (host only): the zero bytes
 * RoutineEncryption appends (never negative). */
int wgcs_padding(size_t packet_size, uint32_t mtu);

/* RoutineEncryption's per-packet work for n packets, asynchronous on stream
 * (NULL: the context's).  Per packet i, with padded = len + padding(len, mtu):
 * writes the header at [off, off + 16), reads the plaintext [off + 16,
 * off + 16 + len), writes ciphertext and tag at [off + 16, off + 32 + padded)
 * (it may read any byte of that range first), and sets d_out_len[i] =
 * 32 + padded.  So the arena must be readable and writable through
 * off + 32 + padded, and no byte outside [off, off + 32 + padded) is written.
 * d_out_len[i] = WGCS_ERR_OUT_OF_RANGE if len > 65535, WGCS_ERR_INVALID_ARG if
 * key >= n_keys; such a packet's bytes are neither read nor written.  n == 0
 * is a no-op. */
int wgcs_aead_seal_batch(wgcs_ctx *ctx, uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                         const wgcs_aead_key *d_keys, uint32_t n_keys, uint32_t n, uint32_t mtu,
                         int32_t *d_out_len, void *stream);

/* RoutineDecryption's per-packet work plus the length trim of
 * RoutineSendToInternet, asynchronous on stream.  Per packet i it reads the
 * message [off, off + len) and writes only inside [off + 16, off + len - 16):
 * the plaintext, in place, when the tag matches, else zeros -- this ABI's
 * contract for what Open leaves of a rejected message; header and tag stay as
 * they were.  d_counter[i] = the counter field (the replay filter stays with
 * the caller; the allowed-source check is wgcs_recv_source_batch).  d_pkt_len[i] =
 *   WGCS_ERR_AUTH              the tag does not match             receive.go:380-383
 *   0                          keepalive (empty plaintext)        :432
 *   the IPv4 total length      if 20 <= it <= plaintext length    :440-449
 *   the IPv6 payload length + 40 in uint16 arithmetic, if <= plaintext length  :460-470
 *   WGCS_ERR_PACKET_TOO_SHORT  any other version nibble, a plaintext shorter
 *                              than its IP header, a length out of range
 *   WGCS_ERR_OUT_OF_RANGE      len < 32 or len > 65535  } nothing read or written,
 *   WGCS_ERR_INVALID_ARG       key >= n_keys            } d_counter[i] = 0
 * n == 0 is a no-op. */
int wgcs_aead_open_batch(wgcs_ctx *ctx, uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                         const wgcs_aead_key *d_keys, uint32_t n_keys, uint32_t n, int32_t *d_pkt_len,
                         uint64_t *d_counter, void *stream);

/* One packet from host memory through the same kernel (staged in device
 * memory; one launch, one wait).  buf[0:16) is the header room, buf[16:16+len)
 * the packet, cap the size of buf; *out_len = 32 + len + padding(len, mtu).
 * WGCS_ERR_OUT_OF_RANGE if len > 65535 or cap < *out_len (buf untouched). */
int wgcs_aead_seal(wgcs_ctx *ctx, const uint8_t key[32], uint32_t remote_index, uint64_t counter,
                   uint8_t *buf, size_t len, size_t cap, uint32_t mtu, size_t *out_len);
/* msg[0:len) is a transport message.  Returns WGCS_OK with the plaintext in
 * msg[16:len-16) and *pkt_len = its trimmed length (0: keepalive), or
 * WGCS_ERR_PACKET_TOO_SHORT likewise decrypted, or WGCS_ERR_AUTH with that
 * range zeroed, or WGCS_ERR_OUT_OF_RANGE (len < 32 or > 65535, msg untouched).
 * *counter = the counter field unless out of range. */
int wgcs_aead_open(wgcs_ctx *ctx, const uint8_t key[32], uint8_t *msg, size_t len, uint64_t *counter,
                   int *pkt_len);

/* ---- peer lookup: allowed-IPs router and session table (device/router.go,
 * device/sessions.go) ----
 * The two data-dependent lookups of the per-packet path: Router.Find on a
 * packet's source or destination address and SessionMap.Get on a transport
 * message's receiver index.  The host keeps the trie (insert / remove as the
 * reference does) and writes a flat image of it; the caller copies the image
 * and the session slots to device memory, as it does the AEAD key table, and
 * the three batch entry points below read them there. */

#define WGCS_PEER_NONE 0xFFFFFFFFu /* Find's nil; never a peer id */

/* Router (router.go:405-495) with caller-chosen uint32 peer ids in place of
 * *Peer.  No context and no device; writers and readers are guarded as the
 * reference's RWMutex guards them.  addr_len is 4 or 16. */
typedef struct wgcs_router wgcs_router;
typedef struct wgcs_prefix {
  uint8_t addr[16]; /* masked to cidr; IPv4 in addr[0:4) */
  uint8_t addr_len; /* 4 or 16 */
  uint8_t cidr;
  uint8_t pad[2];
} wgcs_prefix; /* 20 B */
wgcs_router *wgcs_router_create(void);
void wgcs_router_destroy(wgcs_router *r);
/* Router.Insert (:411-424); the address is masked to cidr (maskSelf, :126-139).
 * INVALID_ARG for an addr_len other than 4 or 16 (the reference panics),
 * cidr > 8 * addr_len or peer == WGCS_PEER_NONE; WGCS_ERR_NOMEM. */
int wgcs_router_insert(wgcs_router *r, const uint8_t *addr, size_t addr_len, uint8_t cidr, uint32_t peer);
/* Router.Remove (:439-457): a no-op unless exactly this prefix is present and is peer's */
int wgcs_router_remove(wgcs_router *r, const uint8_t *addr, size_t addr_len, uint8_t cidr, uint32_t peer);
/* Router.RemoveByPeer (:460-478) */
int wgcs_router_remove_by_peer(wgcs_router *r, uint32_t peer);
/* Router.Find (:426-437): the peer of the longest matching prefix, or
 * WGCS_PEER_NONE (also for a NULL argument or an addr_len other than 4 or 16) */
uint32_t wgcs_router_find(wgcs_router *r, const uint8_t *addr, size_t addr_len);
/* Router.PeerNodes (:481-495): *n = how many prefixes peer has, the first
 * min(*n, cap) of them in out, in the order of the reference's peer.nodes list
 * (insertion order; an exact re-insert moves the prefix to the back) */
int wgcs_router_peer_prefixes(wgcs_router *r, uint32_t peer, wgcs_prefix *out, size_t cap, size_t *n);
/* A flat, position-independent image of both tries: image_size bytes now;
 * write_image fills buf (cap bytes; OUT_OF_RANGE if too small) and sets *len.
 * The format is private to the library.  The device copy must be 16-byte
 * aligned and stays the caller's: write a new image after the router changes. */
size_t wgcs_router_image_size(wgcs_router *r);
int wgcs_router_write_image(wgcs_router *r, uint8_t *buf, size_t cap, size_t *len);
/* Find on an image in host memory (any alignment), the walk the kernels run.
 * INVALID_ARG (*peer = WGCS_PEER_NONE) for bytes that are not an image. */
int wgcs_router_image_find(const uint8_t *buf, size_t len, const uint8_t *addr, size_t addr_len, uint32_t *peer);

/* SessionMap.Get (sessions.go:26-30) as an open-addressed array the caller
 * uploads: slot.key is the session's row in the AEAD key table.  List only
 * sessions that have a keypair (keypair == nil is "not found",
 * receive.go:164-166) and whose keypair has not expired (:168 is host
 * wall-clock state). */
typedef struct wgcs_session_slot {
  uint32_t index; /* the receiver index */
  uint32_t key;   /* 0xFFFFFFFF: the slot is empty */
} wgcs_session_slot;
/* n_slots: a power of two, >= 2 * n and >= 1.  INVALID_ARG for any other
 * n_slots, a key of 0xFFFFFFFF or an index listed twice. */
int wgcs_session_table_build(const uint32_t *indices, const uint32_t *keys, uint32_t n, wgcs_session_slot *slots,
                             uint32_t n_slots);

/* The three batch entry points: ordinary launches, asynchronous on stream
 * (NULL: the context's), n <= 2^28, n == 0 a no-op.  They read the arena and
 * never write it; packets and addresses may sit at any byte offset.
 *
 * The loop body of RoutineReceiveFromPeers (receive.go:145-207).  Message q of
 * d_size[q] bytes is at d_off[q], or at q * stride when d_off is NULL (what
 * wgcs_split_messages_batch writes, with its d_n_out as d_size).  d_type[q] =
 *   0                     size < 32 (nothing read); a handshake type whose
 *                         size is not its own; a transport message whose
 *                         receiver index is not in the table; any other LE32 type
 *   1, 2, 3               initiation of 148 B, response of 92 B, cookie reply of 64 B
 *   4                     a transport message of a listed session
 *   WGCS_ERR_OUT_OF_RANGE size > 65535, or size > stride in the strided form
 *                         (nothing read)
 * and d_pkts[q] = {off, 0, size, key}: key = the session's key for type 4, else
 * 0xFFFFFFFF, which wgcs_aead_open_batch refuses without touching the row; len
 * is 0 for a negative d_type.  d_slots is 4-byte, d_pkts 8-byte aligned. */
int wgcs_recv_classify_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const uint64_t *d_off, uint64_t stride,
                             const int32_t *d_size, uint32_t n, const wgcs_session_slot *d_slots,
                             uint32_t n_slots, wgcs_aead_pkt *d_pkts, int32_t *d_type, void *stream);

/* The allowed-source check of RoutineSendToInternet (receive.go:438-482) on
 * what wgcs_aead_open_batch left.  d_pkt_len[i] <= 0 (a keepalive, any error)
 * passes through to d_verdict[i] with nothing read.  Else the packet is
 * d_pkt_len[i] bytes at d_pkts[i].off + 16: IPv4 of >= 20 B has its source at
 * [12, 16), IPv6 of >= 40 B at [8, 24), anything else is
 * WGCS_ERR_PACKET_TOO_SHORT.  d_verdict[i] = the length if Find(source) ==
 * d_key_peer[d_pkts[i].key], else WGCS_ERR_SOURCE (no route is a mismatch);
 * WGCS_ERR_INVALID_ARG for key >= n_keys or an image that is not one.
 * d_peer (optional) receives Find(source), WGCS_PEER_NONE where none was
 * looked up.  d_verdict may alias d_pkt_len.  d_image is 16-byte aligned. */
int wgcs_recv_source_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                           const int32_t *d_pkt_len, const uint32_t *d_key_peer, uint32_t n_keys, uint32_t n,
                           const uint8_t *d_image, size_t image_bytes, int32_t *d_verdict, uint32_t *d_peer,
                           void *stream);

/* The routing step of RoutineReadFromTUN (send.go:264-293).  The packet of
 * slot q, d_size[q] bytes, starts at (d_off ? d_off[q] : q * stride) + offset
 * (what wgcs_gso_split_batch writes with its offset, with its d_sizes).
 * d_peer[q] = Find(dst) -- IPv4 of >= 20 B: bytes [16, 20), IPv6 of >= 40 B:
 * [24, 40) -- or WGCS_PEER_NONE for size < 1, a shorter packet, any other
 * version nibble, no route or an image that is not one. */
int wgcs_route_dst_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const uint64_t *d_off, uint64_t stride,
                         uint32_t offset, const int32_t *d_size, uint32_t n, const uint8_t *d_image,
                         size_t image_bytes, uint32_t *d_peer, void *stream);

/* ---- per-keypair state: replay filter and send nonce (replay/replay.go,
 * device/receive.go:414-420, device/send.go:383-390) ----
 * The two steps of the per-packet path that are sequential per keypair.  Their
 * state sits in device memory beside the AEAD key table and is indexed by its
 * rows: one wgcs_replay_filter and one uint64 send nonce per key.  The caller
 * zeroes a row (a stream-ordered memset) when it overwrites the key. */

#define WGCS_REJECT_AFTER_MESSAGES 0xFFFFFFFFFFFFDFFFull /* RejectAfterMessages, constants.go:14: the limit of both */

/* replay.Filter: the highest value seen and a ring of 128 blocks of 64 bits
 * (window 127 * 64 = 8,128).  All zero is the empty filter; Reset is a memset. */
typedef struct wgcs_replay_filter {
  uint64_t last;
  uint64_t ring[128];
} wgcs_replay_filter; /* 1,032 B, 8-byte aligned */

/* Filter.Validate / Filter.Reset on a filter in host memory (no context, no
 * device): 1 = accepted, 0 = rejected, WGCS_ERR_INVALID_ARG for NULL. */
int wgcs_replay_validate(wgcs_replay_filter *f, uint64_t value, uint64_t limit);
void wgcs_replay_reset(wgcs_replay_filter *f);

/* The workspace of the two batch entry points below for n rows (or jobs): an
 * upper bound, n <= 2^24.  d_work is the caller's device memory, 16-byte
 * aligned; nothing is allocated inside an enqueue. */
size_t wgcs_keyorder_work_bytes(uint32_t n);

/* keypair.replayFilter.Validate over what wgcs_aead_open_batch left, a few
 * ordinary launches, asynchronous on stream.  Row i takes part if
 * d_pkts[i].key < n_keys and d_pkt_len[i] >= 0 or == WGCS_ERR_PACKET_TOO_SHORT
 * (every message Open decrypted: receive.go:414-420 precedes the trim).  The
 * rows of one key are validated against d_filters[key] in slot order:
 * d_verdict[i] = d_pkt_len[i] if accepted, else WGCS_ERR_REPLAY.  Every other
 * row gets d_verdict[i] = d_pkt_len[i] and touches no filter; filters of keys
 * without a row are not written.  Afterwards each filter is, in all its bytes,
 * what sequential Validate calls leave.  d_verdict may alias d_pkt_len and
 * feeds wgcs_recv_source_batch.  n <= 2^24, n_keys <= 2^24; n == 0 is a no-op;
 * WGCS_ERR_INVALID_ARG (nothing written) for a workspace that is too small. */
int wgcs_replay_batch(wgcs_ctx *ctx, const wgcs_aead_pkt *d_pkts, const int32_t *d_pkt_len,
                      const uint64_t *d_counter, uint32_t n, wgcs_replay_filter *d_filters, uint32_t n_keys,
                      uint64_t limit, int32_t *d_verdict, void *d_work, size_t work_bytes, void *stream);

/* The step between wgcs_route_dst_batch and wgcs_aead_seal_batch (send.go:
 * 383-390): key and nonces of every Tun.Read job, from the outputs of
 * wgcs_gso_split_batch (d_sizes, d_count, d_status; max_segs slots per job)
 * and the peers of its slots.  d_peer_keys (wgcs_session_table_build rows,
 * n_slots a power of two) maps a peer id to its key row.  Job j is kept iff
 * d_status[j] == 0, 1 <= d_count[j] <= max_segs, d_peer[j * max_segs] is a
 * peer found there with a key row < n_keys, and its nonces fit: the kept jobs
 * of a key, in job order, take consecutive nonces from d_send_nonce[key], and
 * a job fits iff its last nonce + 1 <= limit; after one that does not, no
 * later job of that key is kept and d_send_nonce[key] = limit (send.go:386),
 * else it advances by the counts of the kept jobs.
 *   kept job     d_nbufs[j] = d_count[j], d_job_key[j] = key, and row
 *                q = j * max_segs + k, k < d_count[j], of d_pkts is
 *                {q * stride, nonce, (uint32_t)d_sizes[q], key}
 *   dropped job  d_nbufs[j] = 0, d_job_key[j] = 0xFFFFFFFF
 * and every other of the n_jobs * max_segs rows is {q * stride, 0, 0,
 * 0xFFFFFFFF}, which wgcs_aead_seal_batch refuses untouched.  n_jobs <= 2^24,
 * n_jobs * max_segs <= 2^28, n_keys <= 2^24; workspace as above for n_jobs. */
int wgcs_send_assign_batch(wgcs_ctx *ctx, const int32_t *d_sizes, const uint32_t *d_peer, const int32_t *d_count,
                           const int32_t *d_status, uint32_t n_jobs, uint32_t max_segs, uint64_t stride,
                           const wgcs_session_slot *d_peer_keys, uint32_t n_slots, uint64_t *d_send_nonce,
                           uint32_t n_keys, uint64_t limit, wgcs_aead_pkt *d_pkts, int32_t *d_nbufs,
                           uint32_t *d_job_key, void *d_work, size_t work_bytes, void *stream);

/* ---- the Write calls of the receive chain, one per batch and peer
 * (device/receive.go:178-228, :398-504) ----
 * RoutineReceiveIncoming sorts the items of a recvmmsg batch into one
 * container per peer; each peer's RoutineSendToInternet validates its
 * container in slot order, keeps the peer's books for every message that
 * passes the replay filter (rxBytes, validTailPacket, dataPacketReceived,
 * :407-436, :485-494) and hands the packets that are left to one Tun.Write
 * (:483-504).  This step builds those calls, and one accounting row beside
 * each, from what wgcs_recv_source_batch left, so that wgcs_handle_gro_batch
 * can follow on the same stream with no host step between them.
 *
 * Batch b owns rows q in [b * n_msgs, (b + 1) * n_msgs) of d_pkts / d_verdict.
 * Row q is validated iff d_pkts[q].key < n_keys, d_key_peer[key] !=
 * WGCS_PEER_NONE and d_verdict[q] is >= 0, WGCS_ERR_SOURCE or
 * WGCS_ERR_PACKET_TOO_SHORT: the messages that passed replayFilter.Validate
 * (wgcs_replay_batch's participation rule minus its rejects).  It is kept iff
 * it is validated and d_verdict[q] > 0.  Every other row takes no part.
 *
 * The groups of a batch are the distinct peers d_key_peer[key] of its
 * validated rows, ordered by each peer's first validated row (Go leaves the
 * order open: map iteration, one goroutine per peer); the previous and the
 * current keypair of one peer share a group.  Group g of batch b has row
 * c = b * calls_per_batch + g of d_calls and d_groups:
 *   d_calls[c]  = {first, n, offset, gro_flags}: n = the group's kept rows,
 *                 first = b * n_msgs + the kept rows of the groups before it
 *   d_bufs[first + k] = {d_pkts[q].off, offset + d_verdict[q], cap} for the
 *                 group's k-th kept row q in slot order (receive.go:483)
 *   d_groups[c] as below; n == 0 for a peer of keepalives or rejected sources only
 * d_n_groups[b] = the number of groups, d_status[b] = 0.  Every other row the
 * batch owns is written too: unused call rows are {b * n_msgs, 0, offset,
 * gro_flags}, unused group rows {WGCS_PEER_NONE, -1, 0, 0, 0}, and the rows of
 * d_bufs past the batch's kept rows are all zero.  So wgcs_handle_gro_batch
 * runs over all n_batches * calls_per_batch call rows (n == 0 is a no-op
 * there), and afterwards the host reads, per call row, d_groups and GRO's
 * d_status / d_n_write / d_to_write.
 *
 * A refused batch builds nothing: every one of its call and group rows is the
 * unused one and its d_bufs rows are zero; d_n_groups[b] is still the count.
 * d_status[b] = WGCS_ERR_OUT_OF_RANGE if some kept row has offset + verdict >
 * cap (Go would panic slicing), else WGCS_ERR_BATCH_FULL if the batch has more
 * groups than calls_per_batch.
 *
 * One ordinary launch, asynchronous on stream; no workspace, no atomics, the
 * same bytes every time.  The inputs are only read.  WGCS_ERR_INVALID_ARG, and
 * nothing written, unless 1 <= calls_per_batch <= n_msgs <= WGCS_GRO_MAX_CALL,
 * n_batches * n_msgs <= 2^28, 0 <= offset <= cap, no pointer is NULL, d_pkts /
 * d_bufs / d_calls are 16-byte aligned, d_groups 8-byte and the 32-bit arrays
 * 4-byte aligned.  n_batches == 0 is a no-op.
 * wgcs_write_build_host is the same rule on host arrays (no context, no
 * device), array for array. */
#define WGCS_GROUP_DATA 0x1u /* dataPacketReceived, receive.go:436 */
typedef struct wgcs_write_group {
  uint32_t peer;     /* d_key_peer[key] of the group's rows; WGCS_PEER_NONE: unused row */
  int32_t tail;      /* validTailPacket as a row index q of the whole table; -1: unused row */
  uint32_t flags;    /* WGCS_GROUP_DATA: some validated row has d_pkts[q].len > 32 */
  uint32_t n_valid;  /* rows of this peer that passed the replay filter */
  uint64_t rx_bytes; /* sum of d_pkts[q].len over them (= len(item.packet) + MinMessageSize, :431) */
} wgcs_write_group;  /* 24 B, 8-byte aligned */

int wgcs_write_build_batch(wgcs_ctx *ctx, const wgcs_aead_pkt *d_pkts, const int32_t *d_verdict,
                           uint32_t n_msgs, uint32_t n_batches, const uint32_t *d_key_peer, uint32_t n_keys,
                           int32_t offset, uint32_t cap, uint32_t gro_flags, uint32_t calls_per_batch,
                           wgcs_gro_buf *d_bufs, wgcs_gro_call *d_calls, wgcs_write_group *d_groups,
                           int32_t *d_n_groups, int32_t *d_status, void *stream);
int wgcs_write_build_host(const wgcs_aead_pkt *pkts, const int32_t *verdict, uint32_t n_msgs, uint32_t n_batches,
                          const uint32_t *key_peer, uint32_t n_keys, int32_t offset, uint32_t cap,
                          uint32_t gro_flags, uint32_t calls_per_batch, wgcs_gro_buf *bufs, wgcs_gro_call *calls,
                          wgcs_write_group *groups, int32_t *n_groups, int32_t *status);

/* ---- the handshake screen: MAC1, MAC2 and cookie replies (device/cookie.go,
 * device/receive.go:270-287, device/send.go:176-187) ----
 * The denial-of-service defence in front of the Noise handshake.  Every
 * initiation and response carries MAC1 = BLAKE2s-128(mac1_key, msg[0 : len-32])
 * at [len-32, len-16) and MAC2 at [len-16, len).  A message with a wrong MAC1
 * is dropped.  Under load the receiver also wants MAC2 =
 * BLAKE2s-128(cookie, msg[0 : len-16]) with cookie = BLAKE2s-128(secret, source
 * address), and answers a message without it by a cookie reply: the cookie
 * sealed with XChaCha20-Poly1305 under cookie_key, with the message's MAC1 as
 * additional data.  All of it is stateless and per message.
 *
 * Clock and randomness stay with the caller.  The reference compares
 * secretSetAt with CookieRefreshTime (120 s) inside CheckMAC2 and CreateReply
 * (cookie.go:156, :192-203); here the caller draws a new `secret` before it
 * checks a message or enqueues a batch whenever the one it holds is that old.
 * Verdicts and replies are then the reference's: a MAC2 made from a cookie of
 * the old secret fails against the new one, and CreateReply would have
 * refreshed before sealing anyway.  The 24 random nonce bytes of every reply
 * (cookie.go:231) are the caller's as well; nothing here draws randomness or
 * reads a clock.  What comes after a pass is the rate limiter (the
 * wgcs_ratelimit_* section at the end of this header, on the device as well)
 * and the Noise handshake; IsUnderLoad's rule is the host's. */
typedef struct wgcs_cookie_checker { /* 96 B; 4-byte aligned on the device */
  uint8_t mac1_key[32];              /* BLAKE2s-256("mac1----" | pub)   cookie.go:106-109 */
  uint8_t cookie_key[32];            /* BLAKE2s-256("cookie--" | pub)   :112-114 */
  uint8_t secret[32];                /* mac2.secret, the caller's random bytes */
} wgcs_cookie_checker;
typedef struct wgcs_src_addr { /* 20 B: Endpoint.DstToBytes() */
  uint8_t b[18];               /* IP bytes (4 or 16) then LE16 port: netip.AddrPort.MarshalBinary */
  uint8_t len;                 /* 6 or 18 */
  uint8_t pad;
} wgcs_src_addr;

#define WGCS_HS_NONE 0   /* not an initiation or a response: not this step's row */
#define WGCS_HS_PASS 1   /* MAC1 holds, and under load MAC2 too: on to the rate limiter and Noise */
#define WGCS_HS_COOKIE 2 /* under load without a valid MAC2: send the row's cookie reply */

/* Host functions, no context and no device.  msg is a handshake message of len
 * bytes; WGCS_ERR_OUT_OF_RANGE for len < 32 (Go would panic slicing) or
 * len > 65535, WGCS_ERR_INVALID_ARG for a NULL pointer or a source whose len is
 * neither 6 nor 18.
 * CookieChecker.Init and CookieGenerator.Init (cookie.go:102-115, :269-282):
 * both keys from the static public key; secret is zeroed. */
int wgcs_cookie_checker_init(wgcs_cookie_checker *ck, const uint8_t pub[32]);
/* CheckMAC1 (:121-146) and CheckMAC2 (:153-176): 1 or 0.  Tags are compared
 * over all 16 bytes, as hmac.Equal does. */
int wgcs_cookie_check_mac1(const wgcs_cookie_checker *ck, const uint8_t *msg, size_t len);
int wgcs_cookie_check_mac2(const wgcs_cookie_checker *ck, const uint8_t *msg, size_t len, const wgcs_src_addr *src);
/* CreateReply (:184-243) with SendHandshakeCookie's receiver = msg[4:8]
 * (send.go:176-187): the 64-byte MessageCookieReply LE32 3 | LE32 receiver |
 * nonce | sealed cookie. */
int wgcs_cookie_create_reply(const wgcs_cookie_checker *ck, const uint8_t *msg, size_t len, const wgcs_src_addr *src,
                             const uint8_t nonce[24], uint8_t out[64]);
/* AddMACs (:287-314), the sender's side: writes MAC1, copies it to last_mac1
 * (optional), and with a cookie (16 bytes: the caller holds one that is not
 * older than 120 s) writes MAC2; with NULL the MAC2 field is left as it is. */
int wgcs_cookie_add_macs(const uint8_t mac1_key[32], const uint8_t *cookie, uint8_t *msg, size_t len,
                         uint8_t *last_mac1);
/* ConsumeReply (:319-339): 1 and the cookie when the reply opens under
 * cookie_key with last_mac1 as additional data, else 0 (cookie untouched). */
int wgcs_cookie_consume_reply(const uint8_t cookie_key[32], const uint8_t last_mac1[16], const uint8_t reply[64],
                              uint8_t cookie[16]);

/* The screen over the rows that wgcs_recv_classify_batch wrote: an ordinary
 * launch, asynchronous on stream (NULL: the context's), n <= 2^28, n == 0 a
 * no-op.  It reads the arena and never writes it; messages sit at any byte
 * offset, and the arena is read in the aligned 4-byte words that hold a message,
 * so with a 4-byte aligned d_arena it must be readable from align_down(off, 4)
 * through align_up(off + len, 4) (inside the contract of the other batch entry
 * points above).  Row q:
 *   d_type[q] other than 1 or 2   d_verdict[q] = WGCS_HS_NONE, nothing else read
 *                                 (transport rows, cookie replies -- they are
 *                                 wgcs_cookie_consume_batch's, last section --
 *                                 unknown and negative types)
 *   d_pkts[q].len != 148 (type 1) / 92 (type 2)   WGCS_ERR_INVALID_ARG, nothing read
 *   MAC1 of the message at d_pkts[q].off is wrong WGCS_ERR_MAC1
 *   under_load == 0                               WGCS_HS_PASS; MAC2 is not looked at
 *   under_load != 0, with the cookie of d_src[q]:
 *     d_src[q].len neither 6 nor 18               WGCS_ERR_INVALID_ARG
 *     MAC2 matches                                WGCS_HS_PASS
 *     else                                        WGCS_HS_COOKIE, and the 64 bytes at
 *                                                 d_reply + 64 * q are the reply of
 *                                                 wgcs_cookie_create_reply with the
 *                                                 nonce d_nonce[24 * q : 24 * q + 24]
 * The d_reply rows of every other verdict keep what they held.  d_src, d_nonce
 * and d_reply may be NULL when under_load == 0.  d_pkts is 8-byte aligned;
 * d_type, d_checker, d_src, d_nonce, d_verdict and d_reply are 4-byte aligned. */
int wgcs_handshake_screen_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                                const int32_t *d_type, uint32_t n, const wgcs_cookie_checker *d_checker,
                                const wgcs_src_addr *d_src, uint32_t under_load, const uint8_t *d_nonce,
                                int32_t *d_verdict, uint8_t *d_reply, void *stream);

/* ---- X25519 and the consumption of handshake initiations (device/noise.go,
 * device/noise_helpers.go) ----
 * Every initiation that passes the screen costs ConsumeMessageInitiation
 * (noise.go:405-492) one Curve25519 scalar multiplication, 37 BLAKE2s
 * compressions, two ChaCha20-Poly1305 opens and a peer lookup by public key.
 * Everything up to the replay / flood check (:458) is stateless and per
 * message -- no clock, no randomness, no per-peer lock -- and runs here over
 * the batch where it landed.  The comparison with lastTimestamp, the
 * HandshakeInitationRate rule and the handshake-state update (:458-491) need
 * what a row of wgcs_hs_init holds: the host may run them from rows it reads
 * back, or wgcs_handshake_accept_batch (the last section) runs them on the
 * stream against per-peer rows in device memory and writes the descriptors of
 * the next step.  For
 * every initiation accepted, SendHandshakeResponse (send.go:130-169)
 * then costs three more scalar multiplications, a KDF3, an empty seal, AddMACs
 * and the key derivation of BeginSymmetricSession: that runs here as well,
 * over one descriptor per accepted initiation, and leaves the 92-byte response
 * and the two transport keys in device memory (wgcs_handshake_respond_batch
 * below).  Its randomness and its session index are the caller's: the
 * ephemeral private key (newPrivateKey) and the index (sessions.NewIndex, a
 * host map) are fields of the descriptor.  The initiator's half --
 * CreateMessageInitiation and ConsumeMessageResponse with its session keys --
 * runs here too, joined by a table of handshake states in device memory
 * (wgcs_handshake_initiate_batch and wgcs_handshake_finish_batch, the section
 * before the last).  Keypair rotation runs on the stream too (the wgcs_keypairs
 * calls of the last section).  What stays with the host is index allocation;
 * lastSentHandshake, the timers and the consumption of cookie replies have
 * sections of their own further down (wgcs_rekey_*, wgcs_timers_*, wgcs_cookie_*_batch).
 * Nothing here draws randomness or reads a clock. */

/* curve25519.X25519 (RFC 7748 section 5; noise_helpers.go:93-105): the scalar is
 * clamped inside, bit 255 of the point is ignored, a u in [p, 2^255) is
 * reduced, out is fully reduced.  0, or WGCS_ERR_LOW_ORDER with out zeroed for
 * an all-zero result; INVALID_ARG for a NULL pointer.  Host, no device. */
int wgcs_x25519(uint8_t out[32], const uint8_t scalar[32], const uint8_t point[32]);

typedef struct wgcs_noise_responder { /* 96 B, 4-byte aligned on the device */
  uint8_t private_key[32];            /* d.keys.privateKey */
  uint8_t hash0[32];                  /* mixHash(InitialHash, public key)   noise.go:415 */
  uint8_t chain0[32];                 /* InitialChainKey                    noise.go:92 */
} wgcs_noise_responder;
/* Fills r for the static private key; public_key (optional) receives
 * privateKey.publicKey().  INVALID_ARG for a NULL r or private_key. */
int wgcs_noise_responder_init(wgcs_noise_responder *r, const uint8_t private_key[32], uint8_t public_key[32]);

typedef struct wgcs_peer_key { /* 72 B: one row of the table GetPeer reads */
  uint8_t public_key[32];
  uint8_t shared[32]; /* precomputedSharedSecret = X25519(private, public_key) (noise.go:305); zero if that
                         is low order */
  uint32_t peer;      /* caller's peer id, never WGCS_PEER_NONE */
  uint32_t flags;     /* bit 0: peer.isRunning */
} wgcs_peer_key;
#define WGCS_PEER_RUNNING 0x1u
/* The table of n peers: rows sorted by public_key (memcmp order), each with its
 * shared secret under r's private key.  flags may be NULL (every peer
 * running).  INVALID_ARG for a duplicate key, peer == WGCS_PEER_NONE or a NULL
 * argument with n > 0; n == 0 writes nothing. */
int wgcs_peer_keys_build(const wgcs_noise_responder *r, const uint8_t *public_keys /* 32 * n */,
                         const uint32_t *peers, const uint32_t *flags, uint32_t n, wgcs_peer_key *table);
/* the row of public_key, or -1 (also for a NULL argument) */
int wgcs_peer_keys_find(const wgcs_peer_key *table, uint32_t n, const uint8_t public_key[32]);

typedef struct wgcs_hs_init { /* 128 B: what the host needs for noise.go:458-491 */
  uint32_t peer;              /* the table row's peer, WGCS_PEER_NONE until one is found */
  uint32_t sender;            /* LE32 msg[4:8]: hs.remoteIndex */
  uint8_t timestamp[12];      /* the decrypted tai64n timestamp */
  uint8_t pad[12];
  uint8_t hash[32];           /* after mixHash(msg.Timestamp) */
  uint8_t chain_key[32];      /* after the second KDF2 */
  uint8_t ephemeral[32];      /* msg[8:40]: hs.remoteEphemeral */
} wgcs_hs_init;

#define WGCS_HS_CONSUMED 3 /* the initiation is authentic: on to the timestamp and flood rules */

/* The whole stateless part (noise.go:405-457) for one message, on the host: the
 * verdict of wgcs_handshake_consume_batch below for a row of type 1 that
 * passed the screen, with *out filled as that row's d_out.  len != 148 or a
 * NULL pointer (table may be NULL when n_peers == 0): WGCS_ERR_INVALID_ARG. */
int wgcs_noise_consume_initiation(const wgcs_noise_responder *r, const wgcs_peer_key *table, uint32_t n_peers,
                                  const uint8_t *msg, size_t len, wgcs_hs_init *out);
/* The sender's side, CreateMessageInitiation (noise.go:344-403), with the
 * caller's ephemeral private key, timestamp and sender index: the 148 bytes
 * with zero MACs (wgcs_cookie_add_macs fills them), and (optional) the
 * handshake's hash and chaining key after it.  WGCS_ERR_LOW_ORDER where a
 * shared secret is zero (:366-369, :381-383; msg is then zeroed). */
int wgcs_noise_create_initiation(const uint8_t static_private[32], const uint8_t remote_static[32],
                                 const uint8_t ephemeral_private[32], const uint8_t timestamp[12], uint32_t sender,
                                 uint8_t msg[148], uint8_t hash[32], uint8_t chain_key[32]);

/* n scalar multiplications on the device, row q of d_scalars and d_points (32
 * bytes each, 4-byte aligned) into row q of d_out, with d_status[q] = 0 or
 * WGCS_ERR_LOW_ORDER (the row zeroed).  Asynchronous on stream (NULL: the
 * context's); n <= 2^28, n == 0 a no-op. */
int wgcs_x25519_batch(wgcs_ctx *ctx, const uint8_t *d_scalars, const uint8_t *d_points, uint32_t n, uint8_t *d_out,
                      int32_t *d_status, void *stream);

/* ConsumeMessageInitiation up to :457 over the rows the screen passed: an
 * ordinary launch with the screen's contract (asynchronous on stream, n <=
 * 2^28, n == 0 a no-op, the arena only read, in the aligned 4-byte words that
 * hold a message).  d_gate is the screen's d_verdict -- or, under load,
 * wgcs_ratelimit_batch's, which masks rows in it between the two -- or NULL, which
 * selects every row of type 1; d_verdict must not be d_gate.  Row q:
 *   d_type[q] != 1 or d_gate[q] != WGCS_HS_PASS   d_verdict[q] = WGCS_HS_NONE; d_out[q] untouched,
 *                                                 nothing else read
 *   d_pkts[q].len != 148 or LE32 msg[0:4] != 1    WGCS_ERR_INVALID_ARG; d_out[q] untouched   noise.go:406
 *   X25519(private, msg[8:40]) is all zero        WGCS_ERR_LOW_ORDER                          :421-424
 *   msg[40:88] does not open                      WGCS_ERR_AUTH, peer WGCS_PEER_NONE          :427-430
 *   the opened key is not in d_table, its row is
 *   not running or its shared is all zero         WGCS_ERR_NO_PEER                            :432-443
 *   msg[88:116] does not open                     WGCS_ERR_AUTH, peer the row's               :451-455
 *   otherwise                                     WGCS_HS_CONSUMED, the whole d_out[q]
 * For the four failures d_out[q] is zero but for sender and peer (the found
 * row's id, else WGCS_PEER_NONE): no key material is written for a row that
 * failed.  d_responder and d_table are device memory (d_table may be NULL when
 * n_peers == 0); d_pkts is 8-byte aligned, everything else 4-byte aligned.
 * The static private key lives in device memory for as long as d_responder does. */
int wgcs_handshake_consume_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                                 const int32_t *d_type, const int32_t *d_gate, uint32_t n,
                                 const wgcs_noise_responder *d_responder, const wgcs_peer_key *d_table,
                                 uint32_t n_peers, int32_t *d_verdict, wgcs_hs_init *d_out, void *stream);

/* ---- the handshake response (device/noise.go:494-546, :573-604, :636-655,
 * device/cookie.go:287-314, device/send.go:130-169) ---- */

#define WGCS_HS_RESPONDED 4 /* the response is built and both session keys are in place */

/* The responder's side on the host, for one consumed initiation: the work of
 * CreateMessageResponse (noise.go:494-546), of AddMACs under the key
 * BLAKE2s-256("mac1----" | remote_static), and of the responder's
 * BeginSymmetricSession (KDF2(&decrypt, &encrypt, chainKey, nil), :646-651).
 * init is a WGCS_HS_CONSUMED row: its hash, chain_key, ephemeral and sender
 * are read.  The ephemeral private key and local_index (msg.Sender) are the
 * caller's newPrivateKey() and sessions.NewIndex; preshared_key NULL is the
 * all-zero key of a peer without one; cookie (16 bytes) NULL leaves MAC2 zero.
 * msg receives the 92 bytes LE32 2 | LE32 local_index | LE32 init->sender |
 * ephemeral | empty tag | MAC1 | MAC2; send_key (encrypt) and recv_key
 * (decrypt) are optional.  WGCS_ERR_LOW_ORDER where one of the three shared
 * secrets is zero (:520-528): msg and the keys given are then zeroed.
 * INVALID_ARG for a NULL init, remote_static, ephemeral_private or msg. */
int wgcs_noise_create_response(const wgcs_hs_init *init, const uint8_t remote_static[32],
                               const uint8_t preshared_key[32], const uint8_t ephemeral_private[32],
                               uint32_t local_index, const uint8_t cookie[16], uint8_t msg[92], uint8_t send_key[32],
                               uint8_t recv_key[32]);
/* The initiator's side, ConsumeMessageResponse (noise.go:548-620) with its
 * BeginSymmetricSession (KDF2(&encrypt, &decrypt, chainKey, nil), :638-643):
 * under the static private key, the hash, chaining key and ephemeral private
 * key kept from wgcs_noise_create_initiation, and the preshared key (NULL: all
 * zero).  local_index is the index that handshake is registered under, the
 * sender of its initiation: sessions.Get(msg.Receiver) must find it.  MACs are
 * the screen's and are not looked at.  One message on the host; the batch over
 * device-resident states is wgcs_handshake_finish_batch.
 *   len != 92, LE32 msg[0:4] != 2, LE32 msg[8:12] != local_index,
 *   or a NULL static_private, hash, chain_key, ephemeral_private or msg   WGCS_ERR_INVALID_ARG
 *   a shared secret with msg[12:44] is all zero                           WGCS_ERR_LOW_ORDER   :575-584
 *   the empty text msg[44:60] does not open                               WGCS_ERR_AUTH        :599-603
 *   otherwise 0, *sender = LE32 msg[4:8] (hs.remoteIndex), send_key = encrypt, recv_key = decrypt
 * The three outputs are optional; a failure zeroes the keys given and leaves *sender. */
int wgcs_noise_consume_response(const uint8_t static_private[32], const uint8_t hash[32], const uint8_t chain_key[32],
                                const uint8_t ephemeral_private[32], const uint8_t preshared_key[32],
                                uint32_t local_index, const uint8_t *msg, size_t len, uint32_t *sender,
                                uint8_t send_key[32], uint8_t recv_key[32]);

typedef struct wgcs_hs_resp {    /* 80 B, 4-byte aligned: one response to build */
  uint32_t init_row;             /* row of d_init (and of d_gate) */
  uint32_t peer_row;             /* row of d_table: remote static; row of d_psk */
  uint32_t local_index;          /* msg.Sender: the caller's sessions.NewIndex */
  uint32_t send_key, recv_key;   /* rows of d_keys that receive encrypt / decrypt */
  uint32_t flags;                /* bit 0: cookie[] is valid, write MAC2 */
  uint32_t pad[2];
  uint8_t ephemeral_private[32]; /* the caller's newPrivateKey() */
  uint8_t cookie[16];
} wgcs_hs_resp;
#define WGCS_HS_RESP_COOKIE 0x1u

/* wgcs_noise_create_response over n descriptors, one lane each: an ordinary
 * launch, asynchronous on stream (NULL: the context's), n <= 2^28, n == 0 a
 * no-op.  The host's stateful tail (noise.go:458-491) reads the rows of
 * wgcs_handshake_consume_batch back as before and builds one descriptor per
 * initiation it accepts, so the launch is dense.  d_init and d_gate are that
 * call's d_out and d_verdict (d_gate may be NULL: every descriptor is taken);
 * d_table is its peer table, whose row peer_row gives the remote static key;
 * d_psk holds one 32-byte preshared key per table row, or is NULL where no
 * peer has one.  Descriptor j, in this order:
 *   init_row >= n_init, peer_row >= n_peers, send_key or     d_status[j] = WGCS_ERR_INVALID_ARG; nothing else
 *   recv_key >= n_keys, or send_key == recv_key               written or read
 *   d_gate given and d_gate[init_row] != WGCS_HS_CONSUMED     WGCS_HS_NONE; nothing else written
 *   d_init[init_row].peer != d_table[peer_row].peer           WGCS_ERR_NO_PEER; nothing else written
 *   a zero shared secret                          :520-528    WGCS_ERR_LOW_ORDER; the 96 bytes at d_msgs + 96 * j
 *                                                             zeroed, d_keys untouched
 *   otherwise                                                 WGCS_HS_RESPONDED
 * For WGCS_HS_RESPONDED the 92 bytes at d_msgs + 96 * j are the response, MACs
 * included (MAC2 zero without the cookie flag), and the 4 bytes after them are
 * zero; d_keys[send_key] = {encrypt, remote_index = d_init[init_row].sender,
 * pad 0} is ready for wgcs_aead_seal_batch and d_keys[recv_key] = {decrypt,
 * remote_index 0, pad 0} for wgcs_aead_open_batch in the next launch on the
 * stream: no key crosses to the host.  A descriptor that fails writes no key
 * material anywhere.  Two descriptors that name one key row are the caller's
 * error, and which of them wins is unspecified.  d_msgs rows are read back by
 * the lane that wrote them (the MACs).  Everything is 4-byte aligned.
 * d_resp holds the ephemeral private keys for as long as it lives, and d_psk
 * the preshared keys: clear them as the reference clears hs.localEphemeral. */
int wgcs_handshake_respond_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, uint32_t n, const wgcs_hs_init *d_init,
                                 const int32_t *d_gate, uint32_t n_init, const wgcs_peer_key *d_table,
                                 const uint8_t *d_psk, uint32_t n_peers, wgcs_aead_key *d_keys, uint32_t n_keys,
                                 uint8_t *d_msgs, int32_t *d_status, void *stream);

/* ---- the handshake initiator (device/noise.go:344-403, :548-620, :636-662,
 * device/cookie.go:287-314) ----
 * SendHandshakeInitiation and the receipt of its response over device-resident
 * batches.  A table of wgcs_hs_state rows in device memory, one per handshake
 * in flight, joins the two launches: wgcs_handshake_initiate_batch fills a row
 * and wgcs_handshake_finish_batch consumes it, so neither the ephemeral secret
 * nor a transport key of the initiator crosses to the host.  The host keeps
 * what the reference keeps under locks and clocks: sessions.NewIndex and
 * the timers; cookie replies are consumed on the stream as well
 * (wgcs_cookie_consume_batch, the last section); keypair rotation follows on the stream
 * (wgcs_keypairs_begin_initiator_batch), and lastSentHandshake with the
 * decision who needs a handshake is wgcs_rekey_start_batch's (the last
 * section), which writes d_start in device memory. */

#define WGCS_HS_STATE_ZEROED 0    /* handshakeZeroed */
#define WGCS_HS_STATE_INITIATED 1 /* handshakeInitiationCreated */

typedef struct wgcs_hs_state { /* 128 B, 4-byte aligned: one handshake in flight */
  uint32_t state;              /* WGCS_HS_STATE_ZEROED or WGCS_HS_STATE_INITIATED */
  uint32_t local_index;        /* hs.localIndex: the initiation's sender */
  uint32_t peer_row;           /* row of the peer table and of d_psk */
  uint32_t remote_index;       /* msg.Sender of the consumed response, else 0 */
  uint32_t send_key, recv_key; /* rows of d_keys that receive encrypt / decrypt */
  uint32_t claim;              /* 0xFFFFFFFF, or the lowest authentic row of the finish launch in flight */
  uint32_t pad;
  uint8_t hash[32];            /* after mixHash(msg.Timestamp), noise.go:400 */
  uint8_t chain_key[32];       /* after the second KDF2, :384-389 */
  uint8_t ephemeral_private[32];
} wgcs_hs_state;

typedef struct wgcs_hs_start {   /* 96 B, 4-byte aligned: one initiation to build */
  uint32_t state_row;            /* row of d_states that receives the handshake */
  uint32_t peer_row;             /* row of d_table: remote static and precomputedSharedSecret */
  uint32_t local_index;          /* msg.Sender: the caller's sessions.NewIndex */
  uint32_t send_key, recv_key;   /* rows of d_keys the finish step will fill */
  uint32_t flags;                /* bit 0: cookie[] is valid, write MAC2 */
  uint8_t timestamp[12];         /* the caller's tai64n.Now() */
  uint8_t pad0[4];
  uint8_t ephemeral_private[32]; /* the caller's newPrivateKey() */
  uint8_t cookie[16];
  uint8_t pad1[8];
} wgcs_hs_start;
#define WGCS_HS_START_COOKIE 0x1u

#define WGCS_HS_INITIATED 5 /* the initiation is built and its state row is in place */
#define WGCS_HS_FINISHED 6  /* the response is authentic: both session keys are in place, the state is zeroed */

/* CreateMessageInitiation (noise.go:344-403) and AddMACs (cookie.go:287-314)
 * over n descriptors, one lane each: an ordinary launch, asynchronous on
 * stream (NULL: the context's), n <= 2^28, n == 0 a no-op, aligned 4-byte loads
 * and stores only, no randomness drawn and no clock read.  d_static_public is
 * the device's own public key (32 bytes, sealed at :378); d_table holds one
 * wgcs_peer_key row per peer under the device's private key: public_key is the
 * remote static and shared is precomputedSharedSecret, so a lane runs two
 * scalar multiplications (base point x ephemeral, ephemeral x remote static).
 * n_keys only range-checks the key rows, so that the finish step never has to.
 * Descriptor j, in this order:
 *   state_row >= n_states, peer_row >= n_peers, send_key or   d_status[j] = WGCS_ERR_INVALID_ARG; nothing else
 *   recv_key >= n_keys, or send_key == recv_key                written or read
 *   the table row's shared is all zero (:381-383), or          WGCS_ERR_LOW_ORDER; the 160 bytes at d_msgs + 160 * j
 *   X25519(ephemeral, remote static) is (:366-369)             zeroed, the state row untouched
 *   otherwise                                                  WGCS_HS_INITIATED
 * For WGCS_HS_INITIATED the 148 bytes at d_msgs + 160 * j are the initiation
 * with MAC1 under BLAKE2s-256("mac1----" | remote static) and MAC2 (zero
 * without the cookie flag), and the 12 bytes after them are zero; lastMAC1 is
 * bytes [116, 132) of that row, should a cookie reply ever need it.  The state
 * row is written whole: state = WGCS_HS_STATE_INITIATED, local_index,
 * peer_row, send_key and recv_key from the descriptor, remote_index = 0,
 * claim = 0xFFFFFFFF, pad = 0, hash, chain_key and ephemeral_private.  Two
 * descriptors that name one state row are the caller's error, and which of
 * them wins is unspecified.  Everything is 4-byte aligned.  d_start and
 * d_states hold the ephemeral private keys for as long as they live. */
int wgcs_handshake_initiate_batch(wgcs_ctx *ctx, const wgcs_hs_start *d_start, uint32_t n,
                                  const uint8_t *d_static_public, const wgcs_peer_key *d_table, uint32_t n_peers,
                                  uint32_t n_keys, wgcs_hs_state *d_states, uint32_t n_states, uint8_t *d_msgs,
                                  int32_t *d_status, void *stream);

/* ConsumeMessageResponse (noise.go:548-620) and the initiator's
 * BeginSymmetricSession (:636-662) over the rows of a receive batch, with the
 * row gating of wgcs_handshake_consume_batch: asynchronous on stream, n <=
 * 2^28, n == 0 a no-op, the arena only read, d_gate the screen's verdict or
 * NULL (every row of type 2), d_verdict must not be d_gate.  d_responder is
 * the device's own wgcs_noise_responder row, of which only private_key is read; d_slots is
 * a wgcs_session_table_build table that lists local_index -> row of d_states
 * for the handshakes in flight (n_slots a power of two, or 0); d_psk holds one
 * 32-byte preshared key per peer row, or is NULL; d_work is scratch of 64
 * bytes per row.  Row q, in this order, with every state as it stood at launch:
 *   d_type[q] != 2, or d_gate given and d_gate[q] != WGCS_HS_PASS     d_verdict[q] = WGCS_HS_NONE, nothing else read
 *   d_pkts[q].len != 92 or LE32 msg[0:4] != 2                         WGCS_ERR_INVALID_ARG           noise.go:549-551
 *   msg[8:12] not in d_slots, its row >= n_states, that row's
 *   state != WGCS_HS_STATE_INITIATED or its local_index != msg[8:12]  WGCS_ERR_NO_HANDSHAKE          :553-557, :566
 *   the state row's peer_row >= n_peers, or a key row >= n_keys       WGCS_ERR_INVALID_ARG
 *   a shared secret with msg[12:44] is all zero                       WGCS_ERR_LOW_ORDER             :575-584
 *   msg[44:60] does not open                                          WGCS_ERR_AUTH                  :599-603
 *   authentic, but a lower row of this launch is authentic for the
 *   same state row                                                    WGCS_ERR_NO_HANDSHAKE
 *   otherwise                                                         WGCS_HS_FINISHED
 * For WGCS_HS_FINISHED d_keys[send_key] = {encrypt, remote_index = msg.Sender,
 * pad 0} and d_keys[recv_key] = {decrypt, 0, pad 0}, and the state row gets
 * state = WGCS_HS_STATE_ZEROED, remote_index = msg.Sender, claim = 0xFFFFFFFF
 * and zeroed hash, chain_key and ephemeral_private (:658-662).  Every other
 * row writes nothing to d_keys or d_states.  Of several authentic responses to
 * one handshake the lowest row wins whatever the timing: the call is two
 * launches, one that only reads the states, leaves verdict and keys in d_work
 * and takes the minimum of the authentic rows in the state's claim, and one
 * that commits the rows that hold their claim and zeroes d_work, which is all
 * zero when the call's work is done.  The reference, taking the rows in turn,
 * would fail a forged row that follows an authentic one at its state check;
 * here it fails at its tag (WGCS_ERR_AUTH).  d_pkts is 8-byte aligned,
 * everything else 4-byte aligned. */
int wgcs_handshake_finish_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                                const int32_t *d_type, const int32_t *d_gate, uint32_t n,
                                const wgcs_noise_responder *d_responder, const wgcs_session_slot *d_slots,
                                uint32_t n_slots, wgcs_hs_state *d_states, uint32_t n_states, const uint8_t *d_psk,
                                uint32_t n_peers, wgcs_aead_key *d_keys, uint32_t n_keys, uint8_t *d_work,
                                int32_t *d_verdict, void *stream);

/* The two batches on host memory, no context and no device: the same row
 * functions, taken in row order (the finish form in the same two passes), with
 * the same tables and the same outputs.  They are what a host without a GPU
 * calls and what the device's outputs are compared with.  WGCS_ERR_INVALID_ARG
 * for a NULL pointer the device form refuses, n > 2^28 or an n_slots that is
 * not 0 or a power of two; n == 0 a no-op. */
int wgcs_handshake_initiate_host(const wgcs_hs_start *start, uint32_t n, const uint8_t *static_public,
                                 const wgcs_peer_key *table, uint32_t n_peers, uint32_t n_keys, wgcs_hs_state *states,
                                 uint32_t n_states, uint8_t *msgs, int32_t *status);
int wgcs_handshake_finish_host(const uint8_t *arena, const wgcs_aead_pkt *pkts, const int32_t *type,
                               const int32_t *gate, uint32_t n, const wgcs_noise_responder *responder,
                               const wgcs_session_slot *slots, uint32_t n_slots, wgcs_hs_state *states,
                               uint32_t n_states, const uint8_t *psk, uint32_t n_peers, wgcs_aead_key *keys,
                               uint32_t n_keys, uint8_t *work, int32_t *verdict);

/* ---- the responder's stateful tail: timestamp and flood rules
 * (device/noise.go:458-491, tai64n/tai64n.go:54, device/constants.go:33) ----
 * What ConsumeMessageInitiation does after its second AEAD open, between
 * wgcs_handshake_consume_batch and wgcs_handshake_respond_batch on one stream:
 * every WGCS_HS_CONSUMED row is judged against a table of wgcs_hs_peer rows in
 * device memory, the rows that win commit their peer's state, and a dense
 * array of wgcs_hs_resp descriptors comes out that respond takes as it is.  No
 * clock is read and no randomness drawn: the caller passes now, and a pool of
 * tickets (session index, ephemeral private key, two key rows), one per
 * response it is ready to pay for.  The host keeps the timers (lastSentHandshake
 * is wgcs_rekey_responded_batch's), SetEndpointFromPacket from the verdict rows and the index allocation
 * behind the tickets.  The initiator's wgcs_hs_state table is not touched. */

#define WGCS_HS_ACCEPTED 7     /* the initiation won its peer's handshake: its descriptor is written */
#define WGCS_ERR_FLOOD (-25)   /* "handshake flood": within HandshakeInitationRate of the last one  noise.go:469-472 */

#define WGCS_HS_PEER_ZEROED 0   /* handshakeZeroed */
#define WGCS_HS_PEER_CONSUMED 1 /* handshakeInitiationConsumed */
#define WGCS_HS_PEER_SEEN 0x1u   /* wgcs_hs_peer.flags bit 0: last_consumption_ns is set (a non-zero time.Time) */
#define WGCS_HS_PEER_COOKIE 0x2u /* bit 1: cookie[] is valid */

#pragma pack(push, 4)
typedef struct wgcs_hs_peer {    /* 64 B, 4-byte aligned: row r is the responder's handshake of d_table[r] */
  uint8_t last_timestamp[12];    /* hs.lastTimestamp, compared as bytes.Compare does */
  uint32_t state;                /* WGCS_HS_PEER_ZEROED or WGCS_HS_PEER_CONSUMED */
  int64_t last_consumption_ns;   /* hs.lastInitiationConsumption on the caller's monotonic clock; flags bit 0 */
  uint32_t flags;                /* WGCS_HS_PEER_SEEN | WGCS_HS_PEER_COOKIE */
  uint32_t remote_index;         /* hs.remoteIndex: the sender of the last initiation accepted */
  uint32_t claim;                /* 0xFFFFFFFF, or the lowest candidate row of the accept call in flight */
  uint8_t cookie[16];            /* peer.cookieGenerator's cookie (cookie.go:287-314): wgcs_cookie_consume_batch
                                    writes it and flags bit 1, wgcs_cookie_age_batch clears the bit; the
                                    accept and start calls only read them */
  uint8_t pad[12];               /* zero */
} wgcs_hs_peer;
#pragma pack(pop)

typedef struct wgcs_hs_ticket {  /* 48 B, 4-byte aligned: one response the caller is ready to pay for */
  uint32_t local_index;          /* its sessions.NewIndex */
  uint32_t send_key, recv_key;   /* rows of the wgcs_aead_key table */
  uint32_t pad;
  uint8_t ephemeral_private[32]; /* its newPrivateKey() */
} wgcs_hs_ticket;

/* rows[id] = the row of table whose peer is id, WGCS_PEER_NONE for an id no row
 * has: wgcs_hs_init.peer carries the caller's id and not the table row.
 * INVALID_ARG for a row whose peer is >= n_ids, or a NULL table or rows that
 * is needed; a duplicated id keeps its lowest row. */
int wgcs_peer_rows_build(const wgcs_peer_key *table, uint32_t n, uint32_t *rows, uint32_t n_ids);

/* The batch is judged as if its rows were consumed in row order with the clock
 * standing at now_ns (int64 nanoseconds, the caller's monotonic clock); the
 * reference reads the clock per message.  Asynchronous on stream (NULL: the
 * context's), n <= 2^28 and n_tickets <= 2^28, no clock read, no randomness
 * drawn.  d_gate is consume's d_verdict and may not be d_verdict; d_init is
 * its d_out, of which a lane reads only peer, sender and timestamp; d_table is
 * its peer table, d_peer_rows (n_ids words) wgcs_peer_rows_build's rows of it,
 * d_peers one wgcs_hs_peer per table row.  Row q, in this order:
 *   d_gate[q] != WGCS_HS_CONSUMED                      d_verdict[q] = d_gate[q]; nothing else read
 *   d_init[q].peer >= n_ids, d_peer_rows[peer] is
 *   WGCS_PEER_NONE or >= n_peers, or
 *   d_table[row].peer != d_init[q].peer                WGCS_ERR_NO_PEER
 *   otherwise, with last = the peer's last_timestamp and every peer row as it
 *   stood at the call:
 *     the peer floods at the start if flags bit 0 is set and
 *     now_ns - last_consumption_ns <= 20 ms (signed: a clock that went back
 *     floods too).  If it does not, its winner is its lowest row with
 *     timestamp > last.
 *     the winner                                       WGCS_HS_ACCEPTED (WGCS_ERR_BATCH_FULL, below)
 *     timestamp <= the winner's, or <= last without one   WGCS_ERR_REPLAY      noise.go:458, :461-468
 *     any other row                                    WGCS_ERR_FLOOD       :459, :469-472
 * Winners are ranked by row number, ascending, the order in which the
 * reference would have called NewIndex.  The winner of rank j < n_tickets
 * commits (:474-488): last_timestamp = timestamp, last_consumption_ns = now_ns,
 * flags bit 0 set, remote_index = sender, state = WGCS_HS_PEER_CONSUMED; and
 * writes d_resp[j] = {init_row = q, peer_row = its table row, local_index,
 * send_key, recv_key and ephemeral_private of d_tickets[j], flags =
 * WGCS_HS_RESP_COOKIE and the peer row's cookie where its flags bit 1 is set,
 * else 0 and a zero cookie, pads 0}.  A winner of rank >= n_tickets gets
 * WGCS_ERR_BATCH_FULL and leaves its peer's state untouched, so that the
 * initiator's retry is accepted; the other rows of that peer keep the verdicts
 * they had against it.  No other row changes a peer row; claim is 0xFFFFFFFF
 * when the call's work is done, as it must be before it.
 * *d_count = min(winners, n_tickets), the descriptors written.  The tail rows
 * d_resp[*d_count .. n_tickets) are all zero but for init_row = 0xFFFFFFFF,
 * which wgcs_handshake_respond_batch answers with WGCS_ERR_INVALID_ARG,
 * nothing else written or read: launch respond over n_tickets descriptors with
 * d_gate = NULL, without reading the count.  No ticket secret is copied into a
 * tail row.  n == 0 sets *d_count = 0, fills all n_tickets descriptors as the
 * tail and does nothing else.  d_init, d_table, d_peer_rows and d_tickets are
 * only read.  Which wave runs first does not change the outcome: the call is
 * four launches (claim by atomicMin, verdicts and winners per block, a scan of
 * the block counts, commit), over a per-block word of scratch the context
 * owns; a call on another stream of the same context waits for the one before
 * it.  INVALID_ARG for a NULL pointer that is needed (d_count always),
 * d_verdict == d_gate, a count over 2^28 or a pointer that is not 4-byte
 * aligned. */
int wgcs_handshake_accept_batch(wgcs_ctx *ctx, const wgcs_hs_init *d_init, const int32_t *d_gate, uint32_t n,
                                int64_t now_ns, const wgcs_peer_key *d_table, const uint32_t *d_peer_rows,
                                uint32_t n_ids, wgcs_hs_peer *d_peers, uint32_t n_peers,
                                const wgcs_hs_ticket *d_tickets, uint32_t n_tickets, wgcs_hs_resp *d_resp,
                                uint32_t *d_count, int32_t *d_verdict, void *stream);
/* The same contract over host memory, no context and no device: the same row
 * functions in the same passes. */
int wgcs_handshake_accept_host(const wgcs_hs_init *init, const int32_t *gate, uint32_t n, int64_t now_ns,
                               const wgcs_peer_key *table, const uint32_t *peer_rows, uint32_t n_ids,
                               wgcs_hs_peer *peers, uint32_t n_peers, const wgcs_hs_ticket *tickets,
                               uint32_t n_tickets, wgcs_hs_resp *resp, uint32_t *count, int32_t *verdict);

/* ---- keypair rotation: begin-session and first-receive (device/noise.go:664-754,
 * device/sessions.go:70-82, device/receive.go:418-429) ----
 * What puts the keys of a finished handshake to use, between the handshake
 * batches (respond, finish) and the transport batches on one stream: the tail
 * of BeginSymmetricSession -- sessions.AddKeypair, the rotation of previous /
 * current / next with its DeleteSession calls, the initiator's new send key --
 * and ReceivedWithNewKeypair, which promotes the responder's next keypair on
 * the first valid transport packet under it.  Both work on one table of
 * wgcs_keypairs rows in device memory, one per row of the peer table, and on
 * the two slot tables the per-packet path reads: d_slots (receiver index -> key
 * row, wgcs_recv_classify_batch) and d_peer_keys (peer id -> send-key row,
 * wgcs_send_assign_batch).  No slot is inserted or removed: a call only
 * overwrites the key of a slot that exists, so a probe that runs beside it is
 * never broken.  The host registers ahead of time, when it allocates them:
 * every index of a ticket or a wgcs_hs_start goes into d_slots, and every peer
 * id into d_peer_keys, with the key WGCS_SESSION_NO_KEYPAIR.  That key is past
 * every key table (n_keys <= 2^24), so classify hands it on and open, replay,
 * send-assign and the write builder refuse it without touching a row.
 * The host keeps index allocation, SetEndpointFromPacket and
 * SendStagedPackets (from d_rotated), and the reclaiming of tombstoned slots
 * when it rebuilds a table.  Keypair expiry by created_ns is the next
 * section's (wgcs_rekey_recv_gate_batch, wgcs_rekey_send_gate_batch), the
 * timers the one after it (wgcs_timers_rotated_batch reads d_rotated).
 *
 * DeleteSession(x) for a set entry x: the slot of x.local_index in d_slots
 * gets key WGCS_SESSION_NO_KEYPAIR, the 48-byte rows d_keys[x.send_key] and
 * d_keys[x.recv_key] are zeroed (the reference cannot erase key material,
 * keypair.go:12-17), and d_key_peer[x.send_key] = d_key_peer[x.recv_key] =
 * WGCS_PEER_NONE.  For a nil entry it does nothing.  A key row of x at or past
 * n_keys, or an index without a slot, is skipped.  Zeroing a replay filter and
 * a send nonce stays with the caller when it hands a key row out again. */

#define WGCS_SESSION_NO_KEYPAIR 0xFFFFFFFEu /* a wgcs_session_slot key: the index is taken (NewIndex) but has
                                               no keypair yet, or its keypair was deleted: Get finds keypair == nil */
#define WGCS_KEYPAIR_SET 0x1u        /* wgcs_keypair_ref.flags bit 0: the entry holds a keypair; else it is nil and all zero */
#define WGCS_KEYPAIR_INITIATOR 0x2u  /* bit 1: keypair.isInitiator */
#define WGCS_HS_BEGUN 8              /* the keypair is installed and its peer's three entries are rotated */

#pragma pack(push, 4)
typedef struct wgcs_keypair_ref {  /* 24 B */
  uint32_t send_key, recv_key;     /* rows of the wgcs_aead_key table (and of d_send_nonce / d_filters) */
  uint32_t local_index;            /* keypair.localIndex */
  uint32_t flags;
  int64_t created_ns;              /* keypair.createdAt on the caller's clock; written here, read by the wgcs_rekey_* calls */
} wgcs_keypair_ref;
typedef struct wgcs_keypairs {     /* 80 B: row r belongs to d_table[r] */
  wgcs_keypair_ref previous, current, next;
  uint32_t claim;                  /* 0xFFFFFFFF, or the lowest candidate row of the received call in flight */
  uint32_t pad;
} wgcs_keypairs;
#pragma pack(pop)

/* The tail of BeginSymmetricSession (noise.go:664-722) for the handshakes a
 * batch completed, a few ordinary launches, asynchronous on stream (NULL: the
 * context's), n <= 2^24, n_peers <= 2^24, n == 0 a no-op; no clock read.
 * The responder's form runs behind wgcs_handshake_respond_batch: descriptor j
 * is d_resp[j] as accept wrote it and respond consumed it, taken iff
 * d_gate[j] == WGCS_HS_RESPONDED (d_gate is respond's d_status and may not be
 * d_status); its peer_row, local_index, send_key and recv_key are read, its
 * secret fields are not.  The initiator's form runs behind
 * wgcs_handshake_finish_batch: row q of the receive batch is taken iff
 * d_gate[q] == WGCS_HS_FINISHED (finish's d_verdict); the lane reads LE32
 * msg[8:12] in the aligned words that hold it, finds the state row through
 * d_hs_slots (finish's d_slots) and takes peer_row, local_index, send_key and
 * recv_key from that row, which finish left in place; d_states is only read.
 * Descriptor j, in this order:
 *   not taken                                             d_status[j] = WGCS_HS_NONE; nothing else read
 *   initiator: the index is not in d_hs_slots, its state
 *   row >= n_states, or that row's local_index differs    WGCS_ERR_NO_HANDSHAKE
 *   peer_row >= n_peers, a key row >= n_keys, or
 *   send_key == recv_key                                  WGCS_ERR_INVALID_ARG; nothing written
 *   local_index has no slot in d_slots, or its slot's
 *   key is not WGCS_SESSION_NO_KEYPAIR                    WGCS_ERR_NO_HANDSHAKE; nothing written
 *   otherwise                                             WGCS_HS_BEGUN
 * For WGCS_HS_BEGUN, with new = {send_key, recv_key, local_index,
 * WGCS_KEYPAIR_SET | WGCS_KEYPAIR_INITIATOR for the initiator's form, now_ns}:
 * the slot of local_index gets key recv_key (AddKeypair), d_key_peer[send_key]
 * = d_key_peer[recv_key] = d_table[peer_row].peer, and row peer_row of d_kp
 * rotates as noise.go:700-721:
 *   initiator, next set    next = nil, previous = old next, DeleteSession(old current),
 *                          DeleteSession(old previous), current = new
 *   initiator otherwise    previous = old current, DeleteSession(old previous), current = new
 *   responder              next = new, DeleteSession(old next), previous = nil,
 *                          DeleteSession(old previous); current is untouched
 * Whenever current changes, the slot of d_table[peer_row].peer in d_peer_keys
 * gets key current.send_key; a peer id with no slot there is left alone.
 * The descriptors of one peer are applied in descriptor order, as sequential
 * calls would be: the taken descriptors are grouped by peer_row in key order
 * and one lane walks each peer's run.  Two taken descriptors of different
 * peers that name one local_index or one key row are the caller's error, and
 * the outcome is then unspecified.  d_work is wgcs_keyorder_work_bytes(n) of
 * the caller's device memory, 16-byte aligned.  n_slots, n_peer_slots and
 * n_hs_slots are 0 or a power of two; d_pkts is 8-byte aligned, everything
 * else 4-byte aligned.  WGCS_ERR_INVALID_ARG, nothing written, for a NULL
 * pointer that is needed, d_status == d_gate, a count over its bound, a
 * misaligned pointer or a workspace that is too small. */
int wgcs_keypairs_begin_responder_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, const int32_t *d_gate, uint32_t n,
                                        int64_t now_ns, const wgcs_peer_key *d_table, uint32_t n_peers,
                                        wgcs_keypairs *d_kp, wgcs_session_slot *d_slots, uint32_t n_slots,
                                        wgcs_session_slot *d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key *d_keys,
                                        uint32_t *d_key_peer, uint32_t n_keys, int32_t *d_status, void *d_work,
                                        size_t work_bytes, void *stream);
int wgcs_keypairs_begin_initiator_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                                        const int32_t *d_gate, uint32_t n, int64_t now_ns,
                                        const wgcs_session_slot *d_hs_slots, uint32_t n_hs_slots,
                                        const wgcs_hs_state *d_states, uint32_t n_states, const wgcs_peer_key *d_table,
                                        uint32_t n_peers, wgcs_keypairs *d_kp, wgcs_session_slot *d_slots,
                                        uint32_t n_slots, wgcs_session_slot *d_peer_keys, uint32_t n_peer_slots,
                                        wgcs_aead_key *d_keys, uint32_t *d_key_peer, uint32_t n_keys, int32_t *d_status,
                                        void *d_work, size_t work_bytes, void *stream);

/* ReceivedWithNewKeypair (noise.go:725-754) as receive.go:418-429 calls it,
 * behind wgcs_replay_batch on the receive chain's stream: two ordinary
 * launches, asynchronous on stream, n <= 2^28, n == 0 a no-op.  Row i takes
 * part iff d_pkts[i].key < n_keys and d_verdict[i] >= 0 or ==
 * WGCS_ERR_PACKET_TOO_SHORT (decrypted and past the filter; WGCS_ERR_AUTH and
 * WGCS_ERR_REPLAY rows do not), its peer id d_key_peer[key] is < n_ids, and
 * that id's row d_peer_rows[id] is neither WGCS_PEER_NONE nor >= n_peers.  It is
 * a candidate iff that row's next is set and next.recv_key == key.  Of one
 * peer's candidates the lowest row wins, whatever the timing: the first launch
 * takes the minimum of the candidates' row numbers in the row's claim, the
 * second commits the rows that hold their claim and leaves claim = 0xFFFFFFFF,
 * as it must be before the call.  The winning row: d_rotated[i] = 1,
 * DeleteSession(old previous), previous = current, current = next, next = nil,
 * and the peer id's slot in d_peer_keys gets current.send_key, so a
 * wgcs_send_assign_batch that follows on the stream seals under the promoted
 * key.  Every other row of the n gets d_rotated[i] = 0 and changes nothing.
 * d_pkts, d_verdict and d_peer_rows are only read; d_key_peer is read, and
 * written by DeleteSession alone.  d_pkts is 8-byte aligned, everything else
 * 4-byte aligned; n_slots and n_peer_slots are 0 or a power of two. */
int wgcs_keypairs_received_batch(wgcs_ctx *ctx, const wgcs_aead_pkt *d_pkts, const int32_t *d_verdict, uint32_t n,
                                 uint32_t *d_key_peer, uint32_t n_keys, const uint32_t *d_peer_rows, uint32_t n_ids,
                                 wgcs_keypairs *d_kp, uint32_t n_peers, wgcs_session_slot *d_slots, uint32_t n_slots,
                                 wgcs_session_slot *d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key *d_keys,
                                 uint32_t *d_rotated, void *stream);

/* The three on host memory, no context and no device: the same row functions,
 * taken in row order (the received form in the same two passes), with the same
 * tables and the same outputs.  WGCS_ERR_INVALID_ARG for a NULL pointer the
 * device form refuses, a count over its bound or a slot count that is not 0 or
 * a power of two; n == 0 a no-op. */
int wgcs_keypairs_begin_responder_host(const wgcs_hs_resp *resp, const int32_t *gate, uint32_t n, int64_t now_ns,
                                       const wgcs_peer_key *table, uint32_t n_peers, wgcs_keypairs *kp,
                                       wgcs_session_slot *slots, uint32_t n_slots, wgcs_session_slot *peer_keys,
                                       uint32_t n_peer_slots, wgcs_aead_key *keys, uint32_t *key_peer, uint32_t n_keys,
                                       int32_t *status);
int wgcs_keypairs_begin_initiator_host(const uint8_t *arena, const wgcs_aead_pkt *pkts, const int32_t *gate,
                                       uint32_t n, int64_t now_ns, const wgcs_session_slot *hs_slots,
                                       uint32_t n_hs_slots, const wgcs_hs_state *states, uint32_t n_states,
                                       const wgcs_peer_key *table, uint32_t n_peers, wgcs_keypairs *kp,
                                       wgcs_session_slot *slots, uint32_t n_slots, wgcs_session_slot *peer_keys,
                                       uint32_t n_peer_slots, wgcs_aead_key *keys, uint32_t *key_peer, uint32_t n_keys,
                                       int32_t *status);
int wgcs_keypairs_received_host(const wgcs_aead_pkt *pkts, const int32_t *verdict, uint32_t n, uint32_t *key_peer,
                                uint32_t n_keys, const uint32_t *peer_rows, uint32_t n_ids, wgcs_keypairs *kp,
                                uint32_t n_peers, wgcs_session_slot *slots, uint32_t n_slots,
                                wgcs_session_slot *peer_keys, uint32_t n_peer_slots, wgcs_aead_key *keys,
                                uint32_t *rotated);

/* ---- keypair expiry, the rekey rules and the start of a handshake
 * (device/receive.go:80-91, :162-170, device/send.go:84-100, :131-133, :213-227,
 * :368-374, device/constants.go:12-30) ----
 * What looks at a keypair's age and at its send nonce, and what asks for a new
 * handshake, on the streams of the two transport chains and the handshake
 * batches: a gate in each chain that refuses a packet under a keypair past
 * RejectAfterTime or RejectAfterMessages, keepKeyFreshSending and
 * keepKeyFreshReceiving behind them, and a start call that turns the wishes
 * they left into wgcs_hs_start descriptors in device memory, which
 * wgcs_handshake_initiate_batch takes as they are.  A session that ages out on
 * the device is renewed on the device: gate -> start -> initiate -> (peer)
 * consume -> accept -> respond -> begin -> finish -> begin, and the next send
 * batch seals under the new key, with no synchronisation between them.
 *
 * The state is one wgcs_rekey row beside every wgcs_keypairs row.  A lane finds
 * its peer as wgcs_keypairs_received_batch does: peer id -> d_peer_rows[id]
 * (wgcs_peer_rows_build); an id >= n_ids, a row that is WGCS_PEER_NONE or one
 * >= n_peers is "no row".  All clock arithmetic is now_ns - x in signed 64
 * bits; the caller keeps |values| < 2^62.  A clock that went back fires no time
 * rule, and in the start call it counts as "within the timeout".  One clock
 * value serves a whole call, where the reference reads the clock per packet.
 *
 * The host keeps: filling tickets (NewIndex, newPrivateKey, tai64n.Now);
 * sending the d_msgs rows that d_start_peer names.  Cookie ageing
 * (CookieRefreshTime) behind the WGCS_HS_PEER_COOKIE bit is wgcs_cookie_age_batch,
 * which runs on the stream in front of this call (the last section).  handshakeAttempts,
 * the retry timers, timersHandshakeComplete with the clearing of
 * WGCS_REKEY_LAST_MINUTE, and expiredZeroOutKeys are the next section's
 * (wgcs_timers_*): its expire call sets WGCS_REKEY_WANT_NEW_HANDSHAKE and
 * WGCS_REKEY_WANT_RETRY, which d_reasons hands on.  A caller that keeps its
 * timers on the host sets WGCS_REKEY_WANT_HOST and clears
 * WGCS_REKEY_LAST_MINUTE by stream-ordered writes instead.
 *
 * The six calls share their conventions: asynchronous on stream (NULL: the
 * context's), ordinary launches in blocks of 256, no clock read, no randomness
 * drawn, aligned 4-byte or 8-byte accesses only, n == 0 a no-op.
 * WGCS_ERR_INVALID_ARG, nothing written, for a NULL pointer that is needed, a
 * count over its bound or a misaligned pointer: d_pkts, d_groups, d_send_nonce
 * and d_rekey are 8-byte aligned, d_work 16-byte, everything else 4-byte. */

#define WGCS_REJECT_AFTER_TIME_NS 180000000000ll /* RejectAfterTime, constants.go:26 */
#define WGCS_REKEY_AFTER_TIME_NS 120000000000ll  /* RekeyAfterTime, :15 */
#define WGCS_REKEY_TIMEOUT_NS 5000000000ll       /* RekeyTimeout, :18 */
#define WGCS_KEEPALIVE_TIMEOUT_NS 10000000000ll  /* KeepaliveTimeout, :30 */
#define WGCS_REKEY_AFTER_MESSAGES (1ull << 60)   /* RekeyAfterMessages, :12 */
#define WGCS_SESSION_EXPIRED 0xFFFFFFFDu /* a wgcs_aead_pkt key: the keypair is past RejectAfterTime.  Past every
                                            key table, so open refuses it with nothing read and replay, source and
                                            the write builder pass it by */
#define WGCS_ERR_KEY_EXPIRED (-26)   /* no current keypair, or it is past RejectAfterMessages / RejectAfterTime  send.go:369-371 */
#define WGCS_ERR_REKEY_TIMEOUT (-27) /* within RekeyTimeout of lastSentHandshake  send.go:89-98 */
#define WGCS_HS_STARTED 9            /* a wgcs_hs_start descriptor is written for the peer */

#define WGCS_REKEY_LAST_MINUTE 0x1u /* wgcs_rekey.flags bit 0: timers.sentLastMinuteHandshake */

/* wgcs_rekey.want: the reasons a handshake is wanted */
#define WGCS_REKEY_WANT_NO_KEYPAIR 0x01u      /* send.go:369 */
#define WGCS_REKEY_WANT_REJECT_MESSAGES 0x02u /* :370, :385-390 with :419-420 */
#define WGCS_REKEY_WANT_REJECT_TIME 0x04u     /* :371 */
#define WGCS_REKEY_WANT_REKEY_MESSAGES 0x08u  /* :223 */
#define WGCS_REKEY_WANT_REKEY_TIME 0x10u      /* :224 */
#define WGCS_REKEY_WANT_LAST_MINUTE 0x20u     /* receive.go:85-89 */
#define WGCS_REKEY_WANT_HOST 0x40u            /* the timers of a caller that keeps them on the host (expiredNewHandshake,
                                                 expiredResendHandshake), set by a stream-ordered write; the device's
                                                 own are WGCS_REKEY_WANT_NEW_HANDSHAKE and WGCS_REKEY_WANT_RETRY below */

typedef struct wgcs_rekey { /* 16 B, 8-byte aligned: row r belongs to d_table[r] */
  int64_t last_sent_ns;     /* handshake.lastSentHandshake on the caller's monotonic clock; the host
                               initialises it to now - (RekeyTimeout + 1 s), peer.go:180 */
  uint32_t want;            /* WGCS_REKEY_WANT_*, OR-ed in by the calls below; the start call clears it */
  uint32_t flags;           /* WGCS_REKEY_LAST_MINUTE */
} wgcs_rekey;

/* receive.go:162-170, one launch between wgcs_recv_classify_batch and
 * wgcs_aead_open_batch.  Row i takes part iff d_pkts[i].key < n_keys, its peer
 * id d_key_peer[key] has a row, and one of that row's current, previous, next
 * (in that order) is set with recv_key == key.  If now_ns - created_ns of that
 * entry > WGCS_REJECT_AFTER_TIME_NS (Before is strict: equality passes),
 * d_pkts[i].key = WGCS_SESSION_EXPIRED.  Nothing else is written; every other
 * row is untouched.  n <= 2^28. */
int wgcs_rekey_recv_gate_batch(wgcs_ctx *ctx, wgcs_aead_pkt *d_pkts, uint32_t n, int64_t now_ns,
                               const uint32_t *d_key_peer, uint32_t n_keys, const uint32_t *d_peer_rows,
                               uint32_t n_ids, const wgcs_keypairs *d_kp, uint32_t n_peers, void *stream);

/* send.go:368-374, one launch between wgcs_route_dst_batch and
 * wgcs_send_assign_batch.  Job j is taken by send-assign's own rule
 * (d_status_in[j] == 0, 1 <= d_count[j] <= max_segs, peer id
 * d_peer[j * max_segs]) if that peer has a row.  With current of that row:
 *   current is nil                            d_status_out[j] = WGCS_ERR_KEY_EXPIRED, want |= NO_KEYPAIR
 *   d_send_nonce[current.send_key] >= limit   WGCS_ERR_KEY_EXPIRED, want |= REJECT_MESSAGES  } both bits if
 *   now_ns - created_ns >= REJECT_AFTER_TIME  WGCS_ERR_KEY_EXPIRED, want |= REJECT_TIME      } both hold
 * Otherwise, for a current.send_key >= n_keys and for every job not taken,
 * d_status_out[j] = d_status_in[j].  d_status_out may be d_status_in; it is
 * what send-assign then reads as d_status, so a refused job stays staged with
 * the caller.  want is written by atomicOr; d_kp and d_send_nonce are only
 * read.  The rule of :370 is applied per batch and not per SendStagedPackets
 * call.  n_jobs * max_segs <= 2^28. */
int wgcs_rekey_send_gate_batch(wgcs_ctx *ctx, const uint32_t *d_peer, const int32_t *d_count,
                               const int32_t *d_status_in, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                               const uint32_t *d_peer_rows, uint32_t n_ids, const wgcs_keypairs *d_kp,
                               uint32_t n_peers, const uint64_t *d_send_nonce, uint32_t n_keys, uint64_t limit,
                               wgcs_rekey *d_rekey, int32_t *d_status_out, void *stream);

/* keepKeyFreshSending (send.go:213-227, called at :523) and the goto top of
 * :419-420, one launch behind wgcs_send_assign_batch over its outputs; Send is
 * taken to have succeeded.  d_status is the gate's d_status_out.  Job j with
 * status 0, a valid count, a peer row and a set current, with nonce =
 * d_send_nonce[current.send_key] as send-assign left it (a send_key >= n_keys
 * has none, and no nonce rule fires):
 *   kept (d_job_key[j] != 0xFFFFFFFF)   nonce > WGCS_REKEY_AFTER_MESSAGES -> want |= REKEY_MESSAGES;
 *                                       current is initiator and now_ns - created_ns >
 *                                       WGCS_REKEY_AFTER_TIME_NS -> want |= REKEY_TIME
 *   dropped                             nonce >= limit -> want |= REJECT_MESSAGES
 * Nothing but want is written. */
int wgcs_rekey_sent_batch(wgcs_ctx *ctx, const uint32_t *d_peer, const int32_t *d_count, const int32_t *d_status,
                          const uint32_t *d_job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                          const uint32_t *d_peer_rows, uint32_t n_ids, const wgcs_keypairs *d_kp, uint32_t n_peers,
                          const uint64_t *d_send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey *d_rekey,
                          void *stream);

/* keepKeyFreshReceiving (receive.go:80-91, called at :486-488), one launch
 * behind wgcs_write_build_batch over its n_batches * calls_per_batch rows of
 * d_groups (<= 2^28).  A row with tail >= 0 whose peer has a row: if current
 * is set and initiator and now_ns - created_ns > WGCS_REJECT_AFTER_TIME_NS -
 * WGCS_KEEPALIVE_TIMEOUT_NS - WGCS_REKEY_TIMEOUT_NS, then old = atomicOr(&flags,
 * WGCS_REKEY_LAST_MINUTE), and want |= LAST_MINUTE if the bit was clear in
 * old.  There is no per-row output, so the tables are the same whichever
 * group of a peer gets there first. */
int wgcs_rekey_received_batch(wgcs_ctx *ctx, const wgcs_write_group *d_groups, uint32_t n_batches,
                              uint32_t calls_per_batch, int64_t now_ns, const uint32_t *d_peer_rows, uint32_t n_ids,
                              const wgcs_keypairs *d_kp, uint32_t n_peers, wgcs_rekey *d_rekey, void *stream);

/* SendHandshakeResponse's lastSentHandshake (send.go:131-133), one launch
 * behind wgcs_handshake_respond_batch: for descriptor j with d_gate[j] ==
 * WGCS_HS_RESPONDED (respond's d_status) and d_resp[j].peer_row < n_peers,
 * d_rekey[peer_row].last_sent_ns = now_ns.  n <= 2^28. */
int wgcs_rekey_responded_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, const int32_t *d_gate, uint32_t n,
                               int64_t now_ns, wgcs_rekey *d_rekey, uint32_t n_peers, void *stream);

/* SendHandshakeInitiation (send.go:84-100) up to CreateMessageInitiation, one
 * lane per peer row, n_peers <= 2^24, n_tickets <= 2^28.  The tickets are
 * n_tickets prefilled wgcs_hs_start rows (state_row, local_index, send_key,
 * recv_key, timestamp, ephemeral_private; their peer_row, flags, cookie and
 * pads are ignored), the arrangement of accept's tickets.  Peer row r, with
 * w = want as it stood: d_reasons[r] = w, and d_status[r] =
 *   w == 0                                              WGCS_HS_NONE
 *   now_ns - last_sent_ns < WGCS_REKEY_TIMEOUT_NS       WGCS_ERR_REKEY_TIMEOUT; want = 0 (the reference
 *                                                       drops the request, :89-98)
 *   otherwise a candidate; candidates are ranked by row, ascending:
 *     rank k < n_tickets                                WGCS_HS_STARTED: last_sent_ns = now_ns, want = 0,
 *                                                       d_start_peer[k] = r, d_start[k] = ticket k with
 *                                                       peer_row = r, flags = WGCS_HS_START_COOKIE and the
 *                                                       cookie of d_hs_peers[r] where that row's
 *                                                       WGCS_HS_PEER_COOKIE bit is set, else 0 and a zero
 *                                                       cookie; pads 0
 *     rank >= n_tickets                                 WGCS_ERR_BATCH_FULL; the row is untouched, so the
 *                                                       wish survives to the next call
 * *d_count = min(candidates, n_tickets).  The tail rows d_start[*d_count ..
 * n_tickets) are all zero but for state_row = 0xFFFFFFFF, which
 * wgcs_handshake_initiate_batch answers with WGCS_ERR_INVALID_ARG and nothing
 * written; no ticket secret is copied into a tail row, and d_start_peer is
 * WGCS_PEER_NONE there.  So initiate runs over n_tickets rows without reading
 * the count.  n_peers == 0 sets *d_count = 0 and fills all n_tickets rows as
 * the tail.  d_tickets and d_hs_peers are only read.  The call is accept's
 * scheme of launches: verdict and candidates counted per block, a scan of the
 * block counts, commit; which wave runs first does not change a byte of any
 * output.  Its scratch is d_work, wgcs_keyorder_work_bytes(n_peers) bytes of
 * the caller's device memory (WGCS_ERR_INVALID_ARG for fewer): nothing is
 * allocated in an enqueue, and calls on other streams do not wait for it. */
int wgcs_rekey_start_batch(wgcs_ctx *ctx, int64_t now_ns, wgcs_rekey *d_rekey, const wgcs_hs_peer *d_hs_peers,
                           uint32_t n_peers, const wgcs_hs_start *d_tickets, uint32_t n_tickets,
                           wgcs_hs_start *d_start, uint32_t *d_start_peer, uint32_t *d_count, int32_t *d_status,
                           uint32_t *d_reasons, void *d_work, size_t work_bytes, void *stream);

/* The six on host memory, no context and no device: the same row functions,
 * taken in row order (the start form in the same passes), with the same tables
 * and the same outputs.  WGCS_ERR_INVALID_ARG for a NULL pointer the device
 * form refuses or a count over its bound; n == 0 a no-op. */
int wgcs_rekey_recv_gate_host(wgcs_aead_pkt *pkts, uint32_t n, int64_t now_ns, const uint32_t *key_peer,
                              uint32_t n_keys, const uint32_t *peer_rows, uint32_t n_ids, const wgcs_keypairs *kp,
                              uint32_t n_peers);
int wgcs_rekey_send_gate_host(const uint32_t *peer, const int32_t *count, const int32_t *status_in, uint32_t n_jobs,
                              uint32_t max_segs, int64_t now_ns, const uint32_t *peer_rows, uint32_t n_ids,
                              const wgcs_keypairs *kp, uint32_t n_peers, const uint64_t *send_nonce, uint32_t n_keys,
                              uint64_t limit, wgcs_rekey *rekey, int32_t *status_out);
int wgcs_rekey_sent_host(const uint32_t *peer, const int32_t *count, const int32_t *status, const uint32_t *job_key,
                         uint32_t n_jobs, uint32_t max_segs, int64_t now_ns, const uint32_t *peer_rows, uint32_t n_ids,
                         const wgcs_keypairs *kp, uint32_t n_peers, const uint64_t *send_nonce, uint32_t n_keys,
                         uint64_t limit, wgcs_rekey *rekey);
int wgcs_rekey_received_host(const wgcs_write_group *groups, uint32_t n_batches, uint32_t calls_per_batch,
                             int64_t now_ns, const uint32_t *peer_rows, uint32_t n_ids, const wgcs_keypairs *kp,
                             uint32_t n_peers, wgcs_rekey *rekey);
int wgcs_rekey_responded_host(const wgcs_hs_resp *resp, const int32_t *gate, uint32_t n, int64_t now_ns,
                              wgcs_rekey *rekey, uint32_t n_peers);
int wgcs_rekey_start_host(int64_t now_ns, wgcs_rekey *rekey, const wgcs_hs_peer *hs_peers, uint32_t n_peers,
                          const wgcs_hs_start *tickets, uint32_t n_tickets, wgcs_hs_start *start,
                          uint32_t *start_peer, uint32_t *count, int32_t *status, uint32_t *reasons);

/* ---- the peer timers: events, expiry, retry and keepalive
 * (device/timers.go, with device/send.go:85-87, :117-126, :158-160, :193-209,
 * :498-510, device/receive.go:311-312, :339-348, :422-427, :486-494 and
 * device/peer.go:241-252) ----
 * The five timers of a peer and the hooks that arm and cancel them, on the
 * streams of the batches whose rows are the events: six event calls that sit
 * behind the existing batches and read the rows those left in device memory,
 * and one expire call over the peer rows that turns due timers into want bits
 * (so wgcs_rekey_start_batch retries a lost handshake), into keepalive jobs in
 * the layout wgcs_send_assign_batch takes, and into ZeroAndFlushAll's keypair
 * part.  A lost initiation is noticed and retried on the device:
 * initiate -> timers_initiated ... expire -> start -> initiate ->
 * timers_initiated, with no read-back between them.
 *
 * The state is one wgcs_timers row beside every wgcs_keypairs and wgcs_rekey
 * row; peers are found as in the section above.  A timer i is bit i of
 * `pending` and deadline_ns[i]:
 *   Mod(d)      sets the bit and stores deadline_ns[i] = now_ns + d
 *   Del         clears the bit; deadline_ns[i] keeps the value it was last armed
 *               with (0 in a fresh table), which nothing reads while the bit is clear
 *   IsPending   reads the bit
 * One now_ns serves a whole call; all clock arithmetic is signed 64-bit on the
 * caller's clock (|values| < 2^62, keepalive_interval_s <= 65535 as the UAPI
 * allows); a timer is due iff its bit is set and deadline_ns[i] <= now_ns, so a
 * clock that went back fires nothing.  Every `if peer.timersActive()` of
 * timers.go is a test of WGCS_TIMERS_ACTIVE, which only the host writes.
 *
 * No randomness is drawn: where timers.go adds rand.Int64N(
 * RekeyTimeoutJitterMaxMs) milliseconds (:204, :271) the call takes a
 * jitter_seed, and peer row r adds wgcs_timers_jitter_ms(jitter_seed, r) ms, in
 * [0, 334): a fixed integer mix, so every row of one peer in one call computes
 * the same deadline.
 *
 * Several rows of one call may belong to one peer.  A call only ORs bits into
 * or ANDs bits out of the 32-bit words pending and flags (32-bit atomics), no
 * call both sets and clears one bit, and every plain store of a call writes a
 * value that is the same for all rows of the peer; `if !IsPending() { Mod }` is
 * old = atomicOr, and only the lane that found the bit clear stores.  So the
 * table afterwards is, byte for byte, what applying the rows one after the
 * other in row order leaves, whichever wave ran first.
 *
 * The hooks, as the calls below name them (timers.go):
 *   traversal        keepalive_interval_s > 0 and ACTIVE: keepalive.Mod(interval s)        :259-264
 *   packet sent      ACTIVE: sendKeepalive.Del                                             :249-253
 *   packet received  ACTIVE: newHandshake.Del                                              :226-230
 *   data sent        ACTIVE and newHandshake not pending: Mod(15 s + jitter)               :189-221
 *   data received    ACTIVE: sendKeepalive not pending: Mod(10 s), else NEED_ANOTHER       :235-244
 *   initiated        ACTIVE: resendHandshake.Mod(5 s + jitter)                             :268-274
 *   session derived  ACTIVE: zeroOutKeys.Mod(540 s)                                        :291-295
 *   complete         ACTIVE: resendHandshake.Del; attempts = 0; WGCS_REKEY_LAST_MINUTE
 *                    cleared in d_rekey; last_handshake_ns = now_ns                        :279-286
 *
 * The host keeps: index allocation and filling tickets; sending the messages
 * and packets the calls prepared (the endpoint and WGCS_TIMERS_CLEAR_SRC are
 * the wgcs_endpoint_* calls' of the last section, or a host's that keeps the
 * endpoint itself and clears the source when it reads and clears the bit);
 * the staged queue (FlushStagedPackets on
 * WGCS_TIMERS_ACT_FLUSH_STAGED, d_staged); handshake.Clear and
 * sessions.Delete(handshake.localIndex) after WGCS_TIMERS_ACT_ZEROED (cookie
 * ageing and ConsumeReply are the wgcs_cookie_*_batch calls of the last
 * section); the rate limiter's ticker; WGCS_TIMERS_ACTIVE and
 * keepalive_interval_s, by stream-ordered writes (timersStop clears pending).
 *
 * The seven calls share the conventions of the section above: asynchronous on
 * stream (NULL: the context's), ordinary launches in blocks of 256, one lane
 * per row, no clock read, aligned 4-byte or 8-byte accesses only, n == 0 a
 * no-op.  WGCS_ERR_INVALID_ARG, nothing written, for a NULL pointer that is
 * needed, a count over its bound or a misaligned pointer: d_timers, d_rekey,
 * d_pkts and d_groups are 8-byte aligned, d_work 16-byte, everything else
 * 4-byte.  n_peers <= 2^24. */

#define WGCS_TIMER_NEW_HANDSHAKE 0    /* timers.newHandshake: expiredNewHandshake */
#define WGCS_TIMER_RESEND_HANDSHAKE 1 /* timers.resendHandshake */
#define WGCS_TIMER_SEND_KEEPALIVE 2   /* timers.sendKeepalive */
#define WGCS_TIMER_KEEPALIVE 3        /* timers.keepalive: the persistent keepalive */
#define WGCS_TIMER_ZERO_OUT_KEYS 4    /* timers.zeroOutKeys */
#define WGCS_TIMERS_COUNT 5

#define WGCS_TIMERS_ACTIVE 0x1u        /* wgcs_timers.flags: timersActive(); the host's to set */
#define WGCS_TIMERS_NEED_ANOTHER 0x2u  /* timers.needAnotherKeepalive */
#define WGCS_TIMERS_CLEAR_SRC 0x4u     /* markEndpointSrcForClearing: clearSrcOnTx, which the wgcs_endpoint_set_* and _dst_* calls read and clear */
#define WGCS_TIMERS_KEEPALIVE_NOW 0x8u /* a SendKeepalive() is owed, receive.go:348; the expire call emits it */

#define WGCS_TIMERS_JITTER_MAX_MS 334u     /* RekeyTimeoutJitterMaxMs, constants.go:24 */
#define WGCS_TIMERS_MAX_ATTEMPTS 18u       /* MaxHandshakeAttempts, :19 */
#define WGCS_TIMERS_ZERO_KEYS_NS 540000000000ll /* RejectAfterTime * 3, timers.go:100, :293 */

#define WGCS_REKEY_WANT_NEW_HANDSHAKE 0x80u /* wgcs_rekey.want: expiredNewHandshake, SendHandshakeInitiation(false) */
#define WGCS_REKEY_WANT_RETRY 0x100u        /* expiredResendHandshake, SendHandshakeInitiation(true) */

/* d_actions of wgcs_timers_expire_batch: what happened in the row */
#define WGCS_TIMERS_ACT_FIRED(i) (1u << (i)) /* bits 0..4: timer i's body ran */
#define WGCS_TIMERS_ACT_KEEPALIVE 0x20u      /* a keepalive job was written for the peer */
#define WGCS_TIMERS_ACT_DEFERRED 0x40u       /* a keepalive is owed, but n_ka_max jobs were taken: the next call emits it */
#define WGCS_TIMERS_ACT_FLUSH_STAGED 0x80u   /* peer.FlushStagedPackets() is the host's to do */
#define WGCS_TIMERS_ACT_ZEROED 0x100u        /* the three keypairs are deleted: handshake.Clear and its index are the host's */
#define WGCS_TIMERS_ACT_GAVE_UP 0x200u       /* resendHandshake fired past MaxHandshakeAttempts, timers.go:85-101 */

typedef struct wgcs_timers { /* 64 B, 8-byte aligned: row r belongs to d_table[r] */
  int64_t deadline_ns[WGCS_TIMERS_COUNT]; /* when timer i fires, read only while bit i of pending is set */
  int64_t last_handshake_ns;              /* peer.lastHandshake on the caller's clock; 0: never */
  uint32_t pending;                       /* bit i: timers[i].isPending */
  uint32_t attempts;                      /* timers.handshakeAttempts */
  uint32_t flags;                         /* WGCS_TIMERS_* */
  uint32_t keepalive_interval_s;          /* peer.keepaliveInterval */
} wgcs_timers;

/* The jitter of peer row `row` under `seed`, in [0, WGCS_TIMERS_JITTER_MAX_MS):
 * x = seed ^ row * 0x9E3779B9; x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13;
 * x *= 0xC2B2AE35; x ^= x >> 16 (all mod 2^32); the result is (x * 334) >> 32. */
uint32_t wgcs_timers_jitter_ms(uint32_t seed, uint32_t row);

/* send.go:498-510, one launch behind wgcs_send_assign_batch (and
 * wgcs_rekey_sent_batch) over its inputs and d_job_key.  Job j counts iff it
 * was kept (d_job_key[j] != 0xFFFFFFFF), d_status[j] == 0, 1 <= d_count[j] <=
 * max_segs and its peer id d_peer[j * max_segs] has a row.  That row runs
 * traversal and packet sent, and data sent too if some d_sizes[j * max_segs +
 * k] != 0 for k < d_count[j] (a job of keepalives alone has only zero sizes).
 * Only d_timers is written.  n_jobs * max_segs <= 2^28. */
int wgcs_timers_sent_batch(wgcs_ctx *ctx, const int32_t *d_sizes, const uint32_t *d_peer, const int32_t *d_count,
                           const int32_t *d_status, const uint32_t *d_job_key, uint32_t n_jobs, uint32_t max_segs,
                           int64_t now_ns, uint32_t jitter_seed, const uint32_t *d_peer_rows, uint32_t n_ids,
                           wgcs_timers *d_timers, uint32_t n_peers, void *stream);

/* receive.go:486-494, one launch behind wgcs_write_build_batch over its
 * n_batches * calls_per_batch rows of d_groups (<= 2^28).  A row with tail >=
 * 0 whose peer has a row runs traversal and packet received; with
 * WGCS_GROUP_DATA it runs data received: old = atomicOr(&pending,
 * sendKeepalive), the lane that found the bit clear stores now_ns + 10 s, and
 * every other lane sets WGCS_TIMERS_NEED_ANOTHER.  So two data groups of one
 * peer in one call leave the timer armed and the flag set, as the reference's
 * two turns do.  Only d_timers is written. */
int wgcs_timers_received_batch(wgcs_ctx *ctx, const wgcs_write_group *d_groups, uint32_t n_batches,
                               uint32_t calls_per_batch, int64_t now_ns, const uint32_t *d_peer_rows, uint32_t n_ids,
                               wgcs_timers *d_timers, uint32_t n_peers, void *stream);

/* send.go:85-87 and :117-126, behind wgcs_rekey_start_batch and
 * wgcs_handshake_initiate_batch: two launches.  The first, over the n_peers
 * rows: a row whose d_reasons[r] (start's) has any bit other than
 * WGCS_REKEY_WANT_RETRY gets attempts = 0 (!isRetry), even when start answered
 * WGCS_ERR_REKEY_TIMEOUT: :85-87 precede the timeout.  The second, over the
 * n_tickets rows: ticket k with d_start_peer[k] < n_peers (start's; the tail
 * rows hold WGCS_PEER_NONE) and d_init_status[k] == WGCS_HS_INITIATED
 * (initiate's status) runs, on row d_start_peer[k], traversal, packet sent and
 * initiated.  n_tickets <= 2^28 and may be 0; n_peers == 0 is a no-op.  Only
 * d_timers is written. */
int wgcs_timers_initiated_batch(wgcs_ctx *ctx, const uint32_t *d_reasons, const uint32_t *d_start_peer,
                                const int32_t *d_init_status, uint32_t n_tickets, int64_t now_ns,
                                uint32_t jitter_seed, wgcs_timers *d_timers, uint32_t n_peers, void *stream);

/* One launch behind wgcs_handshake_respond_batch: descriptor j with d_gate[j]
 * == WGCS_HS_RESPONDED (respond's d_status) and d_resp[j].peer_row < n_peers
 * runs receive.go:311-312 (traversal, packet received) and then send.go:158-160
 * (session derived, traversal, packet sent).  A descriptor that respond
 * refused runs neither, where the reference had run :311-312 before it tried
 * to respond.  n <= 2^28.  Only d_timers is written. */
int wgcs_timers_responded_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, const int32_t *d_gate, uint32_t n,
                                int64_t now_ns, wgcs_timers *d_timers, uint32_t n_peers, void *stream);

/* receive.go:339-348, one launch behind wgcs_keypairs_begin_initiator_batch
 * over the same rows: row q counts iff d_begun[q] == WGCS_HS_BEGUN (begin's
 * d_status); its peer row is found as begin found it (d_gate[q] ==
 * WGCS_HS_FINISHED, LE32 msg[8:12] -> d_hs_slots -> d_states[row].peer_row),
 * and a row for which that lookup fails or names a peer row >= n_peers is
 * passed by.  The peer row runs traversal, packet received, session derived
 * and complete, and gets WGCS_TIMERS_KEEPALIVE_NOW (:348).  d_timers and the
 * flags of d_rekey are written.  n <= 2^24; n_hs_slots is 0 or a power of two. */
int wgcs_timers_finished_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                               const int32_t *d_gate, const int32_t *d_begun, uint32_t n, int64_t now_ns,
                               const wgcs_session_slot *d_hs_slots, uint32_t n_hs_slots, const wgcs_hs_state *d_states,
                               uint32_t n_states, wgcs_timers *d_timers, wgcs_rekey *d_rekey, uint32_t n_peers,
                               void *stream);

/* receive.go:422-427, one launch behind wgcs_keypairs_received_batch: row i
 * with d_rotated[i] == 1, d_pkts[i].key < n_keys and a peer row for
 * d_key_peer[key] runs complete on that row.  d_timers and the flags of
 * d_rekey are written.  n <= 2^28. */
int wgcs_timers_rotated_batch(wgcs_ctx *ctx, const wgcs_aead_pkt *d_pkts, const uint32_t *d_rotated, uint32_t n,
                              int64_t now_ns, const uint32_t *d_key_peer, uint32_t n_keys, const uint32_t *d_peer_rows,
                              uint32_t n_ids, wgcs_timers *d_timers, wgcs_rekey *d_rekey, uint32_t n_peers,
                              void *stream);

/* The timers' expiry over the peer rows, one lane per row, in the scheme of
 * wgcs_rekey_start_batch: a verdict launch, a one-block scan of per-block
 * counts, a commit launch; scratch is d_work, wgcs_keyorder_work_bytes(n_peers)
 * bytes of the caller's device memory, and nothing is allocated.
 *
 * A row without WGCS_TIMERS_ACTIVE is left alone: d_actions[r] = 0.  An active
 * row fires every timer that is due, in ascending order of deadline, ties by
 * index; a timer's bit is cleared before its body runs (NewTimer's callback),
 * and whatever a body arms is later than now_ns, so at most five bodies run:
 *   newHandshake      flags |= CLEAR_SRC; want |= WGCS_REKEY_WANT_NEW_HANDSHAKE
 *   resendHandshake   attempts > WGCS_TIMERS_MAX_ATTEMPTS: sendKeepalive.Del; actions GAVE_UP |
 *                     FLUSH_STAGED; zeroOutKeys.Mod(540 s) if it is not pending
 *                     otherwise: attempts += 1; flags |= CLEAR_SRC; want |= WGCS_REKEY_WANT_RETRY
 *   sendKeepalive     a keepalive is owed; with NEED_ANOTHER: the flag is cleared and
 *                     sendKeepalive.Mod(10 s)
 *   keepalive         a keepalive is owed iff keepalive_interval_s > 0
 *   zeroOutKeys       DeleteSession (the section above) of d_kp[r]'s current, previous and
 *                     next, which become nil (peer.go:246-251), and the slot of
 *                     d_table[r].peer in d_peer_keys gets WGCS_SESSION_NO_KEYPAIR; actions
 *                     ZEROED | FLUSH_STAGED
 * Each sets WGCS_TIMERS_ACT_FIRED(i).  WGCS_TIMERS_KEEPALIVE_NOW owes a
 * keepalive too.  A row that owes one and has d_staged[r] != 0 (the host has
 * staged packets for the peer, send.go:194; d_staged NULL: nobody has) emits
 * none and its KEEPALIVE_NOW is cleared: SendStagedPackets is the caller's
 * next send batch.  The other owing rows are ranked by row, ascending:
 *   rank k < n_ka_max    job k in send-assign's layout with max_segs == 1: d_ka_peer[k] =
 *                        d_table[r].peer, d_ka_count[k] = 1, d_ka_sizes[k] = 0, d_ka_status[k]
 *                        = 0; KEEPALIVE_NOW is cleared; actions KEEPALIVE
 *   rank >= n_ka_max     KEEPALIVE_NOW is set; actions DEFERRED
 * *d_n_ka = min(owing rows, n_ka_max), and the tail rows [*d_n_ka, n_ka_max)
 * are {WGCS_PEER_NONE, 0, 0, 0}, which wgcs_send_assign_batch drops by their
 * count: the send chain runs over n_ka_max jobs without reading *d_n_ka.  One
 * keepalive per peer and call, however many of its timers owe one.
 * n_peers == 0 sets *d_n_ka = 0 and fills the n_ka_max rows as the tail.
 * d_table and d_staged are only read; want bits are ORed into d_rekey.
 * n_ka_max <= 2^24; n_slots and n_peer_slots are 0 or a power of two.  Two
 * peers whose keypairs name one index or one key row are the caller's error. */
int wgcs_timers_expire_batch(wgcs_ctx *ctx, int64_t now_ns, wgcs_timers *d_timers, wgcs_rekey *d_rekey,
                             const wgcs_peer_key *d_table, uint32_t n_peers, const uint32_t *d_staged,
                             wgcs_keypairs *d_kp, wgcs_session_slot *d_slots, uint32_t n_slots,
                             wgcs_session_slot *d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key *d_keys,
                             uint32_t *d_key_peer, uint32_t n_keys, uint32_t n_ka_max, uint32_t *d_ka_peer,
                             int32_t *d_ka_count, int32_t *d_ka_sizes, int32_t *d_ka_status, uint32_t *d_n_ka,
                             uint32_t *d_actions, void *d_work, size_t work_bytes, void *stream);

/* The seven on host memory, no context and no device: the same row functions,
 * taken in row order (the expire form in the same passes), with the same tables
 * and the same outputs.  WGCS_ERR_INVALID_ARG for a NULL pointer the device
 * form refuses, a count over its bound or a slot count that is not 0 or a power
 * of two; n == 0 a no-op. */
int wgcs_timers_sent_host(const int32_t *sizes, const uint32_t *peer, const int32_t *count, const int32_t *status,
                          const uint32_t *job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                          uint32_t jitter_seed, const uint32_t *peer_rows, uint32_t n_ids, wgcs_timers *timers,
                          uint32_t n_peers);
int wgcs_timers_received_host(const wgcs_write_group *groups, uint32_t n_batches, uint32_t calls_per_batch,
                              int64_t now_ns, const uint32_t *peer_rows, uint32_t n_ids, wgcs_timers *timers,
                              uint32_t n_peers);
int wgcs_timers_initiated_host(const uint32_t *reasons, const uint32_t *start_peer, const int32_t *init_status,
                               uint32_t n_tickets, int64_t now_ns, uint32_t jitter_seed, wgcs_timers *timers,
                               uint32_t n_peers);
int wgcs_timers_responded_host(const wgcs_hs_resp *resp, const int32_t *gate, uint32_t n, int64_t now_ns,
                               wgcs_timers *timers, uint32_t n_peers);
int wgcs_timers_finished_host(const uint8_t *arena, const wgcs_aead_pkt *pkts, const int32_t *gate,
                              const int32_t *begun, uint32_t n, int64_t now_ns, const wgcs_session_slot *hs_slots,
                              uint32_t n_hs_slots, const wgcs_hs_state *states, uint32_t n_states, wgcs_timers *timers,
                              wgcs_rekey *rekey, uint32_t n_peers);
int wgcs_timers_rotated_host(const wgcs_aead_pkt *pkts, const uint32_t *rotated, uint32_t n, int64_t now_ns,
                             const uint32_t *key_peer, uint32_t n_keys, const uint32_t *peer_rows, uint32_t n_ids,
                             wgcs_timers *timers, wgcs_rekey *rekey, uint32_t n_peers);
int wgcs_timers_expire_host(int64_t now_ns, wgcs_timers *timers, wgcs_rekey *rekey, const wgcs_peer_key *table,
                            uint32_t n_peers, const uint32_t *staged, wgcs_keypairs *kp, wgcs_session_slot *slots,
                            uint32_t n_slots, wgcs_session_slot *peer_keys, uint32_t n_peer_slots,
                            wgcs_aead_key *keys, uint32_t *key_peer, uint32_t n_keys, uint32_t n_ka_max,
                            uint32_t *ka_peer, int32_t *ka_count, int32_t *ka_sizes, int32_t *ka_status,
                            uint32_t *n_ka, uint32_t *actions);

/* ---- the rate limiter between the screen and the Noise code
 * (ratelimiter/ratelimiter.go, device/receive.go:283-286) ----
 * Under load every initiation and response that passed MAC2 is charged to a
 * token bucket of its source IP address: 20 packets a second sustained, a burst
 * of 5.  MAC2 proves the source address; the bucket bounds what one proven
 * address may cost the Noise code.  wgcs_ratelimit_batch sits between
 * wgcs_handshake_screen_batch (under_load != 0) and
 * wgcs_handshake_consume_batch on one stream, with nothing read back.
 *
 * The table is n_slots wgcs_rl_entry rows of the caller's memory, n_slots a
 * power of two, 1 <= n_slots <= 2^24, all zero when new.  Open addressing:
 * the entry of an address sits at its home slot
 * wgcs_ratelimit_home_slot(src, n_slots) or at the first slot behind it, going
 * round, that was empty when the address came.  Entries are never deleted in
 * place, so a probe ends at the first empty slot; the cleanup call rebuilds the
 * table without the idle entries instead.  The key of an address is (family,
 * ip): a source of len 6 is family 4 with its 4 bytes then 12 zero bytes, len
 * 18 family 16; the port is not part of it, and 1.2.3.4 and ::ffff:1.2.3.4 are
 * two keys, as they are two netip.Addr values.
 *
 * One now_ns serves a whole call (|now_ns - last_ns| < 2^62; signed 64-bit
 * arithmetic).  The m rows of one address in a call, in row order:
 *   entry found   t0 = min(tokens + (now_ns - last_ns), WGCS_RL_MAX_TOKENS_NS);
 *                 A = t0 >= WGCS_RL_PACKET_COST_NS ? t0 / WGCS_RL_PACKET_COST_NS : 0;
 *                 the first min(m, A) rows pass, the others are refused;
 *                 tokens = t0 - min(m, A) * WGCS_RL_PACKET_COST_NS, last_ns = now_ns
 *                 (a refused call stores the capped tokens and the time too, :113-125)
 *   not found     the first row makes the entry and passes (:96-108), and the
 *                 first 1 + min(m - 1, 4) rows pass;
 *                 tokens = (4 - min(m - 1, 4)) * WGCS_RL_PACKET_COST_NS, last_ns = now_ns
 * which is what m calls of Allow leave when r.now() gives now_ns to each of
 * them.  No address passes more than 5 rows in one call.
 *
 * Deviations from the reference: one clock value per call; the table is
 * bounded, and an address that is new when no slot is free is refused with
 * WGCS_ERR_RATE_TABLE_FULL (Go's map grows); netip.Addr's zone is not part of
 * the key (DstToBytes carries none); rows of one address are charged in row
 * order, where the reference's handshake workers leave the order open.
 * IsUnderLoad and the cleanup ticker -- once a second while the last *d_live
 * or entries_created was not zero -- stay with the host. */
#define WGCS_ERR_RATE_LIMITED (-28)    /* rateLimiter.Allow said no: the message is dropped  receive.go:284-286 */
#define WGCS_ERR_RATE_TABLE_FULL (-29) /* a new address and no free slot in the table: refused (the reference's map is unbounded) */

#define WGCS_RL_PACKET_COST_NS 50000000ll /* packetCost, ratelimiter.go:14 */
#define WGCS_RL_MAX_TOKENS_NS 250000000ll /* maxTokens = packetCost * packetsBurst, :19 */
#define WGCS_RL_CLEANUP_NS 1000000000ll   /* cleanupInterval, :21 */
#define WGCS_RL_CLAIMED 0x80000000u       /* wgcs_rl_entry.state inside a call: | the row that claimed the slot */

typedef struct wgcs_rl_entry { /* 40 B, 8-byte aligned; all zero = empty */
  uint8_t ip[16];              /* 4 address bytes then zeros, or 16 */
  uint32_t state;              /* 0 empty, 1 live; inside a call also WGCS_RL_CLAIMED | row */
  uint32_t family;             /* 4 or 16 */
  int64_t tokens;              /* Entry.tokens, nanoseconds */
  int64_t last_ns;             /* Entry.lastTime on the caller's clock */
} wgcs_rl_entry;

/* The home slot of src's address in a table of n_slots (a power of two; 0 for
 * anything else, a NULL src or a len that is neither 6 nor 18): with w[0..3]
 * the LE32 words of the 16 key bytes, h = 0x811C9DC5 ^ family; for each w[i]: h
 * = (h ^ w[i]) * 0x01000193, h ^= h >> 15; then h ^= h >> 16, h *= 0x85EBCA6B,
 * h ^= h >> 13, h *= 0xC2B2AE35, h ^= h >> 16 (all mod 2^32); h & (n_slots - 1). */
uint32_t wgcs_ratelimit_home_slot(const wgcs_src_addr *src, uint32_t n_slots);

/* One Allow on a table in host memory, no context and no device: 1 allowed, 0
 * refused, WGCS_ERR_RATE_TABLE_FULL, or WGCS_ERR_INVALID_ARG for a NULL
 * pointer, a bad n_slots or a len that is neither 6 nor 18. */
int wgcs_ratelimit_allow(wgcs_rl_entry *table, uint32_t n_slots, const wgcs_src_addr *src, int64_t now_ns);

/* The limiter over the rows of a receive batch.  Row q:
 *   d_gate[q] != WGCS_HS_PASS                 d_verdict[q] = d_gate[q]; nothing else read
 *   d_src[q].len neither 6 nor 18             WGCS_ERR_INVALID_ARG
 *   a new address and no free slot            WGCS_ERR_RATE_TABLE_FULL, every row of it
 *   otherwise                                 WGCS_HS_PASS or WGCS_ERR_RATE_LIMITED by the rule above
 * Initiations and responses are both charged.  When more new addresses come
 * than slots are free, which of them get the slots is unspecified here; the
 * host form gives them out in row order.  d_verdict may be d_gate, and is what
 * wgcs_handshake_consume_batch takes as its d_gate.  d_stats is optional: four
 * words {passed, limited, table_full, entries_created}, written whole.
 *
 * Launches on stream (NULL: the context's), nothing allocated, no clock read:
 * find-or-claim, one lane per row (an empty slot is claimed by a 32-bit
 * compare-and-swap of state, and a claimed slot is compared with the claiming
 * row's d_src, so no lane waits for another); the rows grouped by slot on the
 * key order of wgcs_replay_batch; verdicts and entries, one lane per position,
 * where the first row of a slot's run alone reads and writes the entry.  d_work
 * is wgcs_keyorder_work_bytes(n) bytes of the caller's device memory, 16-byte
 * aligned; d_table is 8-byte aligned, everything else 4-byte.  n <= 2^24; n ==
 * 0 launches nothing but still writes d_stats.  WGCS_ERR_INVALID_ARG, nothing
 * written, for a NULL pointer that is needed, a misaligned one, a bad n_slots,
 * n over its bound or a workspace that is too small. */
int wgcs_ratelimit_batch(wgcs_ctx *ctx, const int32_t *d_gate, const wgcs_src_addr *d_src, uint32_t n,
                         wgcs_rl_entry *d_table, uint32_t n_slots, int64_t now_ns, int32_t *d_verdict,
                         uint32_t *d_stats, void *d_work, size_t work_bytes, void *stream);

/* cleanup() (:77-89) as a rebuild: d_new, which must not overlap d_old, is
 * zeroed on the stream, and every live entry of d_old with now_ns - last_ns <=
 * WGCS_RL_CLEANUP_NS is inserted into it; *d_live = the entries kept, 0 being
 * the reference's "table is empty, stop the ticker".  The caller then uses
 * d_new as the table.  One lane per slot of d_old; where an entry lands among
 * the slots its probe may take depends on the order the lanes ran in. */
int wgcs_ratelimit_cleanup_batch(wgcs_ctx *ctx, const wgcs_rl_entry *d_old, wgcs_rl_entry *d_new, uint32_t n_slots,
                                 int64_t now_ns, uint32_t *d_live, void *stream);

/* The two on host memory, no context and no device: the same row functions in
 * the same passes, rows and slots taken in ascending order. */
int wgcs_ratelimit_batch_host(const int32_t *gate, const wgcs_src_addr *src, uint32_t n, wgcs_rl_entry *table,
                              uint32_t n_slots, int64_t now_ns, int32_t *verdict, uint32_t *stats);
int wgcs_ratelimit_cleanup_host(const wgcs_rl_entry *old_table, wgcs_rl_entry *new_table, uint32_t n_slots,
                                int64_t now_ns, uint32_t *live);

/* ---- the cookie generator: lastMAC1, ConsumeReply and ageing
 * (device/cookie.go:247-339, device/receive.go:246-269) ----
 * The initiator's side of the cookie mechanism.  A peer under load answers a
 * handshake message without MAC2 by a cookie reply; the sender opens it with
 * the MAC1 of the last message it sent that peer as additional data, keeps the
 * cookie, and writes MAC2 with it for the next 120 s.  A table of
 * wgcs_cookie_gen rows in device memory, row r belonging to d_table[r] and
 * d_peers[r], holds what CookieGenerator holds beside the cookie itself.  The
 * cookie and its valid bit stay where wgcs_handshake_accept_batch and
 * wgcs_rekey_start_batch read them: wgcs_hs_peer.cookie and
 * WGCS_HS_PEER_COOKIE.  With the four calls below the round trip runs on one
 * stream with nothing read back:
 *   initiate -> cookie_initiated ... the reply lands -> split -> classify ->
 *   cookie_consume ... cookie_age -> timers expire / start -> initiate (MAC2)
 * and on the responder's side respond -> cookie_responded.  Calls that touch
 * one d_gen or d_peers table are ordered by the caller (one stream), as the
 * calls of the sections above are.
 *
 * The clock is the caller's: one now_ns per call.  The host keeps
 * peer.isRunning (receive.go:259; a reply for a stopped peer is the caller's
 * to keep away), index allocation, and -- if it ever writes a cookie into
 * d_peers itself -- cookie_set_at_ns: a host that writes wgcs_hs_peer.cookie
 * and the bit also writes d_gen[r].cookie_set_at_ns, or does not call
 * wgcs_cookie_age_batch. */
#define WGCS_HS_COOKIE_KEPT 10          /* the cookie reply opened: its peer's row holds a cookie */
#define WGCS_COOKIE_GEN_HAS_MAC1 0x1u   /* wgcs_cookie_gen.flags bit 0: hasLastMAC1 */
#define WGCS_COOKIE_REFRESH_NS 120000000000ll /* CookieRefreshTime, cookie.go:17 */

#pragma pack(push, 4)
typedef struct wgcs_cookie_gen { /* 64 B, 4-byte aligned: row r is the generator of d_table[r] */
  uint8_t cookie_key[32];        /* mac2.encryptionKey: BLAKE2s-256("cookie--" | remote static)  cookie.go:279-281 */
  uint8_t last_mac1[16];         /* mac2.lastMAC1 */
  int64_t cookie_set_at_ns;      /* mac2.cookieSetAt on the caller's monotonic clock */
  uint32_t flags;                /* WGCS_COOKIE_GEN_HAS_MAC1 */
  uint32_t claim;                /* 0 outside a call; inside one the highest row + 1 that wants the row */
} wgcs_cookie_gen;
#pragma pack(pop)

/* CookieGenerator.Init (cookie.go:269-282) per peer row, host code: rows[r] =
 * {cookie_key from table[r].public_key, everything else 0} for r < n.
 * WGCS_ERR_INVALID_ARG for a NULL pointer with n != 0 or n > 2^24. */
int wgcs_cookie_gen_build(const wgcs_peer_key *table, uint32_t n, wgcs_cookie_gen *rows);

/* AddMACs' bookkeeping (cookie.go:301-302) behind wgcs_handshake_initiate_batch
 * and behind wgcs_handshake_respond_batch, over the arrays those calls read and
 * wrote.  Descriptor j takes part iff d_status[j] is WGCS_HS_INITIATED
 * (WGCS_HS_RESPONDED for the responded form) and its peer_row < n_peers; its
 * MAC1 is bytes [116, 132) of d_msgs + 160 * j (bytes [60, 76) of d_msgs + 96 *
 * j).  The outcome is that of taking the descriptors in order: of several for
 * one peer row the highest j leaves its MAC1 in last_mac1, and
 * WGCS_COOKIE_GEN_HAS_MAC1 is set.  Rows no descriptor names change nothing,
 * and nothing but last_mac1 and flags changes (claim is 0 again afterwards).
 *
 * Two launches, asynchronous on stream (NULL: the context's), one lane per
 * descriptor: every one that takes part raises its row's claim to j + 1 (a
 * 32-bit atomic max), then the holder alone stores the 16 bytes and the bit
 * and puts claim back to 0, so no lane writes 16 bytes beside another lane
 * writing the same 16 and the order of the waves does not show.  n <= 2^28, n
 * == 0 or n_peers == 0 a no-op; everything is 4-byte aligned and read and
 * written in 4-byte words.  WGCS_ERR_INVALID_ARG, nothing written, for a NULL
 * pointer that is needed, a misaligned one, a count over its bound, or a d_gen
 * that overlaps d_msgs. */
int wgcs_cookie_initiated_batch(wgcs_ctx *ctx, const wgcs_hs_start *d_start, const int32_t *d_status,
                                const uint8_t *d_msgs, uint32_t n, wgcs_cookie_gen *d_gen, uint32_t n_peers,
                                void *stream);
int wgcs_cookie_responded_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, const int32_t *d_status,
                                const uint8_t *d_msgs, uint32_t n, wgcs_cookie_gen *d_gen, uint32_t n_peers,
                                void *stream);

/* The cookie-reply case of RoutineHandshake (receive.go:246-269) with
 * ConsumeReply (cookie.go:319-339) over the rows that wgcs_recv_classify_batch
 * wrote, with the arena contract of wgcs_handshake_screen_batch: the arena is
 * read and never written, messages sit at any byte offset and are read in the
 * aligned 4-byte words that hold them.  Row q, in this order, with every table
 * as it stood at launch:
 *   d_type[q] != 3                                 d_verdict[q] = WGCS_HS_NONE, nothing else read
 *   d_pkts[q].len != 64 or LE32 msg[0:4] != 3      WGCS_ERR_INVALID_ARG, no table read (unmarshal fails)
 *   no peer row for receiver = LE32 msg[4:8]       WGCS_ERR_NO_PEER (session.peer == nil)
 *   d_gen[row] lacks WGCS_COOKIE_GEN_HAS_MAC1      WGCS_ERR_NO_HANDSHAKE (!hasLastMAC1)
 *   msg[32:64] does not open under cookie_key with nonce msg[8:32]
 *   and last_mac1 as additional data               WGCS_ERR_AUTH
 *   otherwise                                      WGCS_HS_COOKIE_KEPT
 * The peer row of a receiver (d.indexTable.Lookup): (1) if receiver is in
 * d_hs_slots with a row < n_states and d_states[row].local_index == receiver,
 * in whatever state, it is that row's peer_row -- a handshake we initiated;
 * (2) else, if receiver is in d_slots with a key < n_keys, d_key_peer[key] is
 * an id < n_ids and d_peer_rows[id] < n_peers, it is d_peer_rows[id] -- a
 * response we sent, which wgcs_keypairs_begin_responder_batch registered; (3)
 * anything else is no peer: WGCS_SESSION_NO_KEYPAIR, an empty slot, a row at or
 * past n_peers.
 *
 * Every row that opens for one peer gets WGCS_HS_COOKIE_KEPT, and the highest
 * row's cookie is the one that stands (the reference, taking them in turn,
 * overwrites): d_peers[row].cookie = that cookie, d_peers[row].flags |=
 * WGCS_HS_PEER_COOKIE and no other bit, d_gen[row].cookie_set_at_ns = now_ns.
 * last_mac1 and WGCS_COOKIE_GEN_HAS_MAC1 stay, as in the reference.  No other
 * row of any table changes.
 *
 * Two launches on stream: the first opens every reply, leaves the cookie in
 * d_work and claims the peer's row by an atomic max of q + 1; the second
 * commits the holders, puts claim back to 0 and zeroes all of d_work, so no
 * cookie outlives the call there.  d_work is 16 bytes of the caller's device
 * memory per row.  No clock is read and no randomness drawn.  n <= 2^28, n ==
 * 0 a no-op; slot counts are 0 or a power of two; d_pkts is 8-byte aligned,
 * everything else 4-byte.  WGCS_ERR_INVALID_ARG, nothing written, for a NULL
 * pointer that is needed, a misaligned one, a count over its bound, or when two
 * of d_work, d_verdict, d_gen and d_peers overlap. */
int wgcs_cookie_consume_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                              const int32_t *d_type, uint32_t n, int64_t now_ns,
                              const wgcs_session_slot *d_hs_slots, uint32_t n_hs_slots, const wgcs_hs_state *d_states,
                              uint32_t n_states, const wgcs_session_slot *d_slots, uint32_t n_slots,
                              const uint32_t *d_key_peer, uint32_t n_keys, const uint32_t *d_peer_rows, uint32_t n_ids,
                              wgcs_cookie_gen *d_gen, wgcs_hs_peer *d_peers, uint32_t n_peers, void *d_work,
                              int32_t *d_verdict, void *stream);

/* The check AddMACs makes per message (cookie.go:306) with the clock standing
 * at now_ns for the batch, one lane per peer row, on the stream in front of
 * wgcs_handshake_accept_batch and wgcs_rekey_start_batch:
 *   WGCS_HS_PEER_COOKIE set and now_ns - cookie_set_at_ns > WGCS_COOKIE_REFRESH_NS
 *                      that bit of d_peers[r].flags is cleared and nothing else
 *   any other row      untouched
 * The difference is signed (|now_ns - cookie_set_at_ns| < 2^63): a clock that
 * went back keeps the cookie, as time.Since would.  n_peers <= 2^24, 0 a no-op;
 * WGCS_ERR_INVALID_ARG for a NULL or misaligned table or two that overlap. */
int wgcs_cookie_age_batch(wgcs_ctx *ctx, int64_t now_ns, const wgcs_cookie_gen *d_gen, wgcs_hs_peer *d_peers,
                          uint32_t n_peers, void *stream);

/* The four on host memory, no context and no device: the same row functions
 * in the same passes, rows taken in ascending order.  Tables, d_msgs and the
 * work rows are 4-byte aligned; the arena is read by bytes and never outside a
 * message. */
int wgcs_cookie_initiated_host(const wgcs_hs_start *start, const int32_t *status, const uint8_t *msgs, uint32_t n,
                               wgcs_cookie_gen *gen, uint32_t n_peers);
int wgcs_cookie_responded_host(const wgcs_hs_resp *resp, const int32_t *status, const uint8_t *msgs, uint32_t n,
                               wgcs_cookie_gen *gen, uint32_t n_peers);
int wgcs_cookie_consume_host(const uint8_t *arena, const wgcs_aead_pkt *pkts, const int32_t *type, uint32_t n,
                             int64_t now_ns, const wgcs_session_slot *hs_slots, uint32_t n_hs_slots,
                             const wgcs_hs_state *states, uint32_t n_states, const wgcs_session_slot *slots,
                             uint32_t n_slots, const uint32_t *key_peer, uint32_t n_keys, const uint32_t *peer_rows,
                             uint32_t n_ids, wgcs_cookie_gen *gen, wgcs_hs_peer *peers, uint32_t n_peers, void *work,
                             int32_t *verdict);
int wgcs_cookie_age_host(int64_t now_ns, const wgcs_cookie_gen *gen, wgcs_hs_peer *peers, uint32_t n_peers);

/* ---- the staged queue: peer.qus.staged on the device (device/send.go:331-426) ----
 * The packets a peer cannot send yet -- no current keypair, or one past its
 * limits -- wait in a ring per peer in the caller's device memory, beside the
 * other per-peer tables: row r belongs to d_table[r], and a peer id finds its
 * row through d_peer_rows / n_ids as in the rekey section.
 *   uint32_t d_len[n_peers]              packets staged for the peer.  A plain word array: it is
 *                                        what wgcs_timers_expire_batch takes as d_staged
 *   uint32_t d_head[n_peers]             ring position of the oldest packet
 *   uint32_t d_lost[n_peers]             packets evicted or flushed so far (PutQuOutItems), modulo 2^32
 *   int32_t  d_slot_size[n_peers * cap]  the size of every slot's packet; 0 is a keepalive
 *   uint8_t  d_ring[n_peers * cap * stride]  slot s = r * cap + pos holds its packet at s * stride + 16,
 *                                        the send arena's layout with the header room in front
 * cap is a power of two in [1, 1024], n_peers <= 2^24, n_peers * cap <= 2^28,
 * stride a multiple of 16 (the arena's, the ring's and d_out's alike), d_ring,
 * d_arena and d_out 16-byte aligned.  An all-zero state is the empty queue.
 * The unit is the packet, not the reference's group of one Read's items, and
 * eviction is oldest first per packet (the reference bounds a peer at
 * QuStagedSize = 128 groups; cap = 128 is the recommended ring).
 *
 * All three calls are asynchronous on stream (NULL: the context's), ordinary
 * launches, nothing allocated in an enqueue, no clock read.  Every ring slot
 * and every output job has one writing lane group and the words of a peer one
 * lane, so which wave runs first changes no byte of any output.
 * WGCS_ERR_INVALID_ARG, nothing written, for a NULL pointer that is needed, a
 * misaligned one, a cap that is no power of two, a count over its bound,
 * d_ring overlapping d_arena or d_out, or scratch that is too small. */

#define WGCS_STAGED_RELEASED 11        /* the peer's staged packets are jobs of the output table, its ring is empty */
#define WGCS_STAGED_NONE 0xFFFFFFFFu    /* d_where: the slot is not staged */
#define WGCS_STAGED_EVICTED 0xFFFFFFFEu /* d_where: staged and evicted within the call, never copied */

/* StagePackets (send.go:331-350) and the re-staging of :402-407, behind
 * wgcs_send_assign_batch over the job table the chain just ran on.  Job j is
 * staged iff d_status_in[j] == 0, 1 <= d_count[j] <= max_segs, its peer
 * d_peer[j * max_segs] has a row, and either the gate refused it
 * (d_status_out[j] == WGCS_ERR_KEY_EXPIRED) or send-assign dropped it
 * (d_status_out[j] == 0 and d_job_key[j] == 0xFFFFFFFF).  d_status_in and
 * d_status_out are the gate's two arrays (two arrays: a gate that ran in
 * place leaves no status_in to read).  A segment q = j * max_segs + k, k <
 * d_count[j], is a packet of the job iff 0 <= d_sizes[q] and 16 + d_sizes[q] +
 * 32 <= stride -- what wgcs_aead_seal_batch needs of a slot, stride being a
 * multiple of 16; other segments are passed by.
 *
 * The packets of one peer in the call, in job order and then segment order,
 * have ranks 0 .. m - 1.  With L = d_len[r] and head = d_head[r] before the
 * call, rank k goes to ring position (head + L + k) & (cap - 1).  If L + m >
 * cap the oldest L + m - cap packets are evicted, old ones first, then those of
 * this call with k < m - cap, which are not copied at all: d_head advances and
 * d_lost grows by that number, and d_len = min(L + m, cap).  Bytes [16, 16 +
 * size) of the source slot are copied to the same range of the ring slot and
 * d_slot_size[slot] = size; no other byte of d_ring or d_slot_size is written.
 * d_where[q], for every q < n_jobs * max_segs, is the ring slot index,
 * WGCS_STAGED_NONE or WGCS_STAGED_EVICTED.  The job table is only read.
 *
 * The jobs of one peer are ranked through the key order that replay,
 * send-assign and the rate limiter use, the peer row as the key; d_work is
 * wgcs_keyorder_work_bytes(n_jobs) bytes of scratch, 16-byte aligned.  The
 * first launch counts the staged jobs into d_work; on a zero count -- most
 * send batches -- the later launches return at once.  n_jobs <= 2^24,
 * n_jobs * max_segs <= 2^28, n_jobs == 0 a no-op. */
int wgcs_staged_stage_batch(wgcs_ctx *ctx, const uint8_t *d_arena, uint64_t stride, const int32_t *d_sizes,
                            const uint32_t *d_peer, const int32_t *d_count, const int32_t *d_status_in,
                            const int32_t *d_status_out, const uint32_t *d_job_key, uint32_t n_jobs, uint32_t max_segs,
                            const uint32_t *d_peer_rows, uint32_t n_ids, uint32_t *d_len, uint32_t *d_head,
                            uint32_t *d_lost, int32_t *d_slot_size, uint8_t *d_ring, uint32_t n_peers, uint32_t cap,
                            uint32_t *d_where, void *d_work, size_t work_bytes, void *stream);

/* SendStagedPackets (send.go:363-426) over the peer rows, wherever the
 * reference calls it: at the head of a send batch, behind
 * wgcs_keypairs_begin_initiator_batch and behind wgcs_keypairs_received_batch.
 * Peer row r, d_status[r] =
 *   d_len[r] == 0                            WGCS_HS_NONE
 *   the send gate's rule fails (:368-374: current nil, d_send_nonce[current.send_key] >= limit,
 *   now_ns - created_ns >= WGCS_REJECT_AFTER_TIME_NS)
 *                                            WGCS_ERR_KEY_EXPIRED; the gate's want bits are OR-ed into
 *                                            d_rekey[r].want, the ring is untouched
 *   otherwise a candidate of weight d_len[r]; candidates are taken by row, ascending, P the weights
 *   of the candidates below:
 *     P + d_len[r] <= n_out_max              WGCS_STAGED_RELEASED: the packet at ring position
 *                                            (head + i) & (cap - 1) becomes job k = P + i of the
 *                                            output table, its bytes at [k * stride + 16, + size) of
 *                                            d_out, d_out_peer[k] = d_table[r].peer, d_out_count[k] = 1,
 *                                            d_out_sizes[k] = size, d_out_status[k] = 0; then
 *                                            d_len[r] = d_head[r] = 0
 *     otherwise                              WGCS_ERR_BATCH_FULL, the row untouched; P only grows, so
 *                                            every candidate behind the first that does not fit is
 *                                            deferred too
 * *d_n_out = the jobs written, and rows [*d_n_out, n_out_max) of the output
 * table are {WGCS_PEER_NONE, 0, 0, 0}, which send-assign drops by their count:
 * the chain behind (send-assign with max_segs == 1, wgcs_rekey_sent_batch,
 * wgcs_timers_sent_batch, seal, and wgcs_staged_stage_batch again for what
 * send-assign dropped at the nonce limit) runs over n_out_max jobs without
 * reading the count.  No byte of d_out outside a job's [16, 16 + size) is
 * written.  The candidates are ranked by the count-scan-rank scheme of accept,
 * start and expire with the packets of a row as its weight; d_work is
 * wgcs_keyorder_work_bytes(n_peers) bytes of scratch.  n_out_max <= 2^28;
 * n_peers == 0 sets *d_n_out = 0 and fills all n_out_max rows as the tail. */
int wgcs_staged_release_batch(wgcs_ctx *ctx, int64_t now_ns, const wgcs_peer_key *d_table, const wgcs_keypairs *d_kp,
                              const uint64_t *d_send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey *d_rekey,
                              uint32_t *d_len, uint32_t *d_head, const int32_t *d_slot_size, const uint8_t *d_ring,
                              uint32_t n_peers, uint32_t cap, uint64_t stride, uint32_t n_out_max, uint8_t *d_out,
                              uint32_t *d_out_peer, int32_t *d_out_count, int32_t *d_out_sizes, int32_t *d_out_status,
                              uint32_t *d_n_out, int32_t *d_status, void *d_work, size_t work_bytes, void *stream);

/* FlushStagedPackets (send.go:352-361), one lane per peer row over the
 * d_actions of wgcs_timers_expire_batch: a row with
 * WGCS_TIMERS_ACT_FLUSH_STAGED gets d_lost += d_len, d_len = 0, d_head = 0.
 * d_actions == NULL flushes every row (peer.Stop, peer.go:259).  n_peers == 0
 * a no-op. */
int wgcs_staged_flush_batch(wgcs_ctx *ctx, const uint32_t *d_actions, uint32_t *d_len, uint32_t *d_head,
                            uint32_t *d_lost, uint32_t n_peers, void *stream);

/* The three on host memory, no context and no device: the same row functions,
 * rows taken in row order, the same state and the same outputs.  The stage
 * form's work is 16 * n_jobs bytes, 8-byte aligned (wgcs_keyorder_work_bytes
 * (n_jobs) covers it); the release form needs none.  WGCS_ERR_INVALID_ARG, and
 * nothing written, for what the device forms refuse. */
int wgcs_staged_stage_host(const uint8_t *arena, uint64_t stride, const int32_t *sizes, const uint32_t *peer,
                           const int32_t *count, const int32_t *status_in, const int32_t *status_out,
                           const uint32_t *job_key, uint32_t n_jobs, uint32_t max_segs, const uint32_t *peer_rows,
                           uint32_t n_ids, uint32_t *len, uint32_t *head, uint32_t *lost, int32_t *slot_size,
                           uint8_t *ring, uint32_t n_peers, uint32_t cap, uint32_t *where, void *work,
                           size_t work_bytes);
int wgcs_staged_release_host(int64_t now_ns, const wgcs_peer_key *table, const wgcs_keypairs *kp,
                             const uint64_t *send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey *rekey,
                             uint32_t *len, uint32_t *head, const int32_t *slot_size, const uint8_t *ring,
                             uint32_t n_peers, uint32_t cap, uint64_t stride, uint32_t n_out_max, uint8_t *out,
                             uint32_t *out_peer, int32_t *out_count, int32_t *out_sizes, int32_t *out_status,
                             uint32_t *n_out, int32_t *status);
int wgcs_staged_flush_host(const uint32_t *actions, uint32_t *len, uint32_t *head, uint32_t *lost, uint32_t n_peers);

/* ---- the peer endpoints: roaming, sticky source, send destination
 * (conn/bind.go:308-319, :398-430, conn/sticky.go:46-94, device/peer.go:195-221,
 * :281-297, device/receive.go:314, :335, :487) ----
 * peer.endpoint on the device.  A table of wgcs_endpoint rows in the caller's
 * device memory, row r belonging to d_table[r], holds where each peer is: the
 * AddrPort its last authentic packet came from and the sticky source
 * (IP_PKTINFO / IPV6_PKTINFO control message) that packet arrived on.  Beside
 * it is one uint32_t claim word per row, 0 outside a call as
 * wgcs_cookie_gen.claim is.  clearSrcOnTx is WGCS_TIMERS_CLEAR_SRC of the
 * peer's wgcs_timers row, which wgcs_timers_expire_batch sets.
 *
 *   recv        the endpoint of every packet slot of a receive batch, and the
 *               dense address table the screen and the rate limiter take:
 *               split -> endpoint_recv -> classify -> screen -> ratelimit with
 *               nothing read back                                bind.go:308-319
 *   set_*       SetEndpointFromPacket at its three live call sites:
 *               behind write_build (:487), accept (:314) and finish (:335)
 *   dst_*       the part of Peer.Send in front of bind.Send: the destination
 *               of every send job, initiation and response, with ClearSrc
 *                                                                peer.go:201-211
 *   coalesce_messages_dst   coalesceMessages with one address family per batch
 *
 * Rows are canonical -- zero bytes at and past src_len, zero pad -- so tables
 * can be compared whole; a row is read and written as sixteen 4-byte words.
 * The call at receive.go:423 (rotation) needs no call of its own: the
 * rotating packet is a valid one, so validTailPacket >= its index and :487
 * overwrites the endpoint in the same container turn.
 *
 * The host keeps: turning recvmmsg's Addr into the wgcs_src_addr of each
 * landed message; the UAPI's peer.endpoint.val = endpoint (uapi.go:325), a
 * stream-ordered write of a table row; device/sticky.go's route listener, a
 * stream-ordered OR of WGCS_TIMERS_CLEAR_SRC; txBytes, which it raises by
 * d_tx_bytes when its send succeeds; and sending.
 *
 * Conventions are those of the timers and cookie-generator sections:
 * asynchronous on stream (NULL: the context's), ordinary launches in blocks of
 * 256, one lane per row, aligned 4-byte accesses only, nothing allocated, no
 * clock read, a row count of 0 a no-op.  WGCS_ERR_INVALID_ARG, nothing
 * written, for a NULL pointer that is needed, a misaligned one (d_timers,
 * d_pkts, d_groups and d_tx_bytes 8-byte, everything else 4-byte), a count
 * over its bound (rows 2^28, n_peers 2^24), or where two of a call's tables
 * and outputs overlap, or one of them and recv's inputs or a set call's d_ep. */
typedef struct wgcs_endpoint {   /* 64 B, 4-byte aligned */
  wgcs_src_addr dst;             /* AddrPort; dst.len == 0: no endpoint (peer.endpoint.val == nil) */
  uint8_t src_len;               /* len(NetEndpoint.src): 0, 32 or 40 */
  uint8_t pad[3];                /* zero */
  uint8_t src[40];               /* NetEndpoint.src; zero at and past src_len */
} wgcs_endpoint;
#define WGCS_ERR_NO_ENDPOINT (-30) /* "no known endpoint for peer"  peer.go:202-205 */

/* The tail of ReceiveIPvX (bind.go:308-319) over n_batches recvmmsg batches of
 * n_msgs slots, behind wgcs_split_messages_batch or on its own.  Slot q = b *
 * n_msgs + s: d_addr[q] is the address recvmmsg left in msgs[s].Addr, d_from is
 * split's d_src (NULL: every slot carries its own), d_size its d_n_out, and
 * msgs[s].OOB[:NN] is the d_nn[q] bytes at d_oob + q * oob_stride (oob_stride
 * a multiple of 4; a d_nn[q] outside [0, oob_stride] reads as no control).
 *   d_size[q] == 0, or d_from[q] outside [-1, n_msgs)   d_ep[q] all zero
 *   otherwise   dst = d_addr[q] (d_from[q] == -1) or d_addr[b * n_msgs + d_from[q]], its 20 bytes as
 *               given; src = getSrcFromControl of slot q's own control buffer
 * splitMessages moves Addr alone (bind.go:570), so a split packet has the
 * address of its source message and the sticky source of its own slot.
 * getSrcFromControl walks the control messages as wgcs_get_gso_size does,
 * stops at the first IPPROTO_IP/IP_PKTINFO (0/8: 32 bytes) or
 * IPPROTO_IPV6/IPV6_PKTINFO (41/50: 40 bytes) and leaves its 16 header bytes as
 * received, then the data from byte 16 on, cut to the room left, zeros behind
 * a shorter one; a parse error leaves the source empty.  d_addr_out (may be
 * NULL) gets dst of every slot: wgcs_handshake_screen_batch's and
 * wgcs_ratelimit_batch's d_src.  n_batches * n_msgs <= 2^28. */
int wgcs_endpoint_recv_batch(wgcs_ctx *ctx, const wgcs_src_addr *d_addr, const int32_t *d_from, const int32_t *d_size,
                             const uint8_t *d_oob, uint32_t oob_stride, const int32_t *d_nn, uint32_t n_msgs,
                             uint32_t n_batches, wgcs_endpoint *d_ep, wgcs_src_addr *d_addr_out, void *stream);

/* SetEndpointFromPacket (peer.go:281-286) over the rows of the call in front;
 * d_ep is wgcs_endpoint_recv_batch's, n_rows rows.  Two launches: every
 * candidate raises d_claim[peer row] to its index + 1 by a 32-bit atomic max;
 * then the holder alone stores the 64 bytes of its source row into
 * d_table[peer row], clears WGCS_TIMERS_CLEAR_SRC in d_timers[peer row].flags
 * by an atomic AND and puts the claim back to 0.  The table afterwards is what
 * taking the rows in ascending order leaves.  A candidate whose source row has
 * a dst.len that is neither 6 nor 18 is none.  d_ep may not overlap d_table.
 *   received  :487, behind wgcs_write_build_batch over its n_batches * calls_per_batch rows: a
 *             row with 0 <= tail < n_rows whose peer id has a row below n_peers takes d_ep[tail]
 *   accepted  :314, behind wgcs_handshake_accept_batch over its n_tickets descriptors: one with
 *             init_row < n_rows and peer_row < n_peers takes d_ep[init_row], whatever
 *             wgcs_handshake_respond_batch answers later (the tail rows carry 0xFFFFFFFF)
 *   finished  :335, behind wgcs_handshake_finish_batch: row q with d_gate[q] == WGCS_HS_FINISHED
 *             whose peer row is found as wgcs_timers_finished_batch finds it takes d_ep[q];
 *             begin's status is not read.  n <= 2^24; n_hs_slots 0 or a power of two */
int wgcs_endpoint_set_received_batch(wgcs_ctx *ctx, const wgcs_write_group *d_groups, uint32_t n_batches,
                                     uint32_t calls_per_batch, const wgcs_endpoint *d_ep, uint32_t n_rows,
                                     const uint32_t *d_peer_rows, uint32_t n_ids, wgcs_endpoint *d_table,
                                     uint32_t *d_claim, wgcs_timers *d_timers, uint32_t n_peers, void *stream);
int wgcs_endpoint_set_accepted_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, uint32_t n_tickets,
                                     const wgcs_endpoint *d_ep, uint32_t n_rows, wgcs_endpoint *d_table,
                                     uint32_t *d_claim, wgcs_timers *d_timers, uint32_t n_peers, void *stream);
int wgcs_endpoint_set_finished_batch(wgcs_ctx *ctx, const uint8_t *d_arena, const wgcs_aead_pkt *d_pkts,
                                     const int32_t *d_gate, uint32_t n, const wgcs_session_slot *d_hs_slots,
                                     uint32_t n_hs_slots, const wgcs_hs_state *d_states, uint32_t n_states,
                                     const wgcs_endpoint *d_ep, wgcs_endpoint *d_table, uint32_t *d_claim,
                                     wgcs_timers *d_timers, uint32_t n_peers, void *stream);

/* Peer.Send in front of bind.Send (peer.go:201-211).  Entry j:
 *   takes no part                        d_dst[j] all zero, d_dst_v6[j] = 0, d_dst_status[j] = 0
 *   its peer row has dst.len == 0        a zero row, 0 and WGCS_ERR_NO_ENDPOINT; the peer's
 *                                        WGCS_TIMERS_CLEAR_SRC stays (Send returns before it)
 *   otherwise                            d_dst[j] = the peer's row, with src_len 0 and a zero src if
 *                                        the peer's WGCS_TIMERS_CLEAR_SRC is set; d_dst_v6[j] = 1 iff
 *                                        dst.len == 18 (Is6(), v4-mapped included); status 0
 * and afterwards every such peer whose flag was set has the source of its
 * table row cleared and the flag too: the result of taking the entries in
 * order.  Two launches, read and clear, so that no lane reads a row another
 * lane is clearing.  The outputs may not overlap d_table or d_timers.
 *   jobs       behind wgcs_aead_seal_batch, in front of coalesce.  Job j takes part by the rule of
 *              wgcs_timers_sent_batch (kept, status 0, 1 <= count <= max_segs, the peer of
 *              d_peer[j * max_segs] has a row).  One without an endpoint also gets d_nbufs[j] = 0,
 *              so coalesce builds no message for it; its nonces are spent, as in the reference.
 *              d_tx_bytes[j] = the sum of d_lens[j * max_segs + k] (negative: 0) over k < d_nbufs[j]
 *              (within [0, max_segs]) for a job with a destination, else 0: the operand of
 *              peer.go:213-218.  n_jobs * max_segs <= 2^28
 *   initiated  over wgcs_handshake_initiate_batch's d_start and d_status == WGCS_HS_INITIATED
 *   responded  over wgcs_handshake_respond_batch's d_resp and d_status == WGCS_HS_RESPONDED
 *              both with peer_row < n_peers, the rule of the two wgcs_cookie_*ed_batch calls */
int wgcs_endpoint_dst_jobs_batch(wgcs_ctx *ctx, const uint32_t *d_peer, const int32_t *d_count, const int32_t *d_status,
                                 const uint32_t *d_job_key, uint32_t n_jobs, uint32_t max_segs, const int32_t *d_lens,
                                 int32_t *d_nbufs, const uint32_t *d_peer_rows, uint32_t n_ids,
                                 wgcs_endpoint *d_table, wgcs_timers *d_timers, uint32_t n_peers, wgcs_endpoint *d_dst,
                                 int32_t *d_dst_v6, int32_t *d_dst_status, uint64_t *d_tx_bytes, void *stream);
int wgcs_endpoint_dst_initiated_batch(wgcs_ctx *ctx, const wgcs_hs_start *d_start, const int32_t *d_status, uint32_t n,
                                      wgcs_endpoint *d_table, wgcs_timers *d_timers, uint32_t n_peers,
                                      wgcs_endpoint *d_dst, int32_t *d_dst_v6, int32_t *d_dst_status, void *stream);
int wgcs_endpoint_dst_responded_batch(wgcs_ctx *ctx, const wgcs_hs_resp *d_resp, const int32_t *d_status, uint32_t n,
                                      wgcs_endpoint *d_table, wgcs_timers *d_timers, uint32_t n_peers,
                                      wgcs_endpoint *d_dst, int32_t *d_dst_v6, int32_t *d_dst_status, void *stream);

/* wgcs_coalesce_messages_batch with the address family per batch: batch b
 * coalesces up to maxIPv6PayloadLen if d_dst_v6[b] != 0, else up to
 * maxIPv4PayloadLen (bind.go:615-618); d_dst_v6 is wgcs_endpoint_dst_jobs_batch's
 * and is read once per batch.  A kernel instantiation of its own: the
 * existing entry runs the code it ran. */
int wgcs_coalesce_messages_dst_batch(wgcs_ctx *ctx, uint8_t *d_bufs, uint64_t buf_stride, uint32_t buf_cap,
                                     const int32_t *d_caps, const int32_t *d_lens, const int32_t *d_nbufs,
                                     uint32_t max_bufs, uint32_t n_batches, const int32_t *d_dst_v6, int32_t *d_n_msgs,
                                     int32_t *d_msg_first, int32_t *d_msg_len, int32_t *d_msg_gso, void *stream);

/* The seven on host memory, no context and no device, array for array: the
 * same row functions in the same passes, rows taken in ascending order.
 * WGCS_ERR_INVALID_ARG, nothing written, for what the device forms refuse. */
int wgcs_endpoint_recv_host(const wgcs_src_addr *addr, const int32_t *from, const int32_t *size, const uint8_t *oob,
                            uint32_t oob_stride, const int32_t *nn, uint32_t n_msgs, uint32_t n_batches,
                            wgcs_endpoint *ep, wgcs_src_addr *addr_out);
int wgcs_endpoint_set_received_host(const wgcs_write_group *groups, uint32_t n_batches, uint32_t calls_per_batch,
                                    const wgcs_endpoint *ep, uint32_t n_rows, const uint32_t *peer_rows, uint32_t n_ids,
                                    wgcs_endpoint *table, uint32_t *claim, wgcs_timers *timers, uint32_t n_peers);
int wgcs_endpoint_set_accepted_host(const wgcs_hs_resp *resp, uint32_t n_tickets, const wgcs_endpoint *ep,
                                    uint32_t n_rows, wgcs_endpoint *table, uint32_t *claim, wgcs_timers *timers,
                                    uint32_t n_peers);
int wgcs_endpoint_set_finished_host(const uint8_t *arena, const wgcs_aead_pkt *pkts, const int32_t *gate, uint32_t n,
                                    const wgcs_session_slot *hs_slots, uint32_t n_hs_slots, const wgcs_hs_state *states,
                                    uint32_t n_states, const wgcs_endpoint *ep, wgcs_endpoint *table, uint32_t *claim,
                                    wgcs_timers *timers, uint32_t n_peers);
int wgcs_endpoint_dst_jobs_host(const uint32_t *peer, const int32_t *count, const int32_t *status,
                                const uint32_t *job_key, uint32_t n_jobs, uint32_t max_segs, const int32_t *lens,
                                int32_t *nbufs, const uint32_t *peer_rows, uint32_t n_ids, wgcs_endpoint *table,
                                wgcs_timers *timers, uint32_t n_peers, wgcs_endpoint *dst, int32_t *dst_v6,
                                int32_t *dst_status, uint64_t *tx_bytes);
int wgcs_endpoint_dst_initiated_host(const wgcs_hs_start *start, const int32_t *status, uint32_t n,
                                     wgcs_endpoint *table, wgcs_timers *timers, uint32_t n_peers, wgcs_endpoint *dst,
                                     int32_t *dst_v6, int32_t *dst_status);
int wgcs_endpoint_dst_responded_host(const wgcs_hs_resp *resp, const int32_t *status, uint32_t n, wgcs_endpoint *table,
                                     wgcs_timers *timers, uint32_t n_peers, wgcs_endpoint *dst, int32_t *dst_v6,
                                     int32_t *dst_status);

#ifdef __cplusplus
}
#endif
#endif /* WGCSUM_H */
