"""ctypes binding of the in-tree C ABI library (wireguard_amd/libwgcsum.so).

The library is the product: every checksum / GSO / GRO byte is processed by
its gfx950 HIP kernels.  There is no Python or CPU fallback -- if the library
is missing or no device is present, loading or context creation raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WGCS_LIB") or os.path.join(_HERE, "libwgcsum.so")  # WGCS_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "wgcsum.h")

# status codes (include/wgcsum.h)
OK = 0
ERR_INVALID_ARG = -1
ERR_SHORT_BUFFER = -2
ERR_TOO_MANY_SEGMENTS = -3
ERR_INVALID_OFFSET = -4
ERR_UNSUPPORTED_GSO = -5
ERR_IP_GSO_MISMATCH = -6
ERR_BAD_IP_VERSION = -7
ERR_PACKET_TOO_SHORT = -8
ERR_TCP_HDR_LEN = -9
ERR_HDR_LEN = -10
ERR_CSUM_OFFSET = -11
ERR_READ_OVERFLOW = -12
ERR_OUT_OF_RANGE = -13
ERR_BATCH_FULL = -14
ERR_NOT_READY = -15
ERR_CMSG = -16
ERR_SPLIT_OVERFLOW = -17
ERR_AUTH = -18
ERR_SOURCE = -19
ERR_REPLAY = -20
ERR_MAC1 = -21
ERR_LOW_ORDER = -22
ERR_NO_PEER = -23
ERR_NO_HANDSHAKE = -24
ERR_FLOOD = -25
ERR_KEY_EXPIRED = -26
ERR_REKEY_TIMEOUT = -27
ERR_RATE_LIMITED = -28
ERR_RATE_TABLE_FULL = -29
ERR_NO_ENDPOINT = -30
ERR_HIP = -100
ERR_NOMEM = -101
ERR_NO_DEVICE = -102

MODE_FOLD, MODE_L4_FILL, MODE_VALIDATE, MODE_PARTIAL, MODE_IP4HDR = 0, 1, 2, 3, 4
F_INPLACE = 0x1
PKT_V6 = 0x01
PEER_NONE = 0xFFFFFFFF  # Router.Find's nil
REJECT_AFTER_MESSAGES = 0xFFFFFFFFFFFFDFFF  # constants.go:14
HS_NONE, HS_PASS, HS_COOKIE = 0, 1, 2  # wgcs_handshake_screen_batch's verdicts
HS_CONSUMED = 3  # wgcs_handshake_consume_batch's
HS_RESPONDED = 4  # wgcs_handshake_respond_batch's
HS_RESP_COOKIE = 0x1  # wgcs_hs_resp.flags: cookie[] is valid
HS_INITIATED = 5  # wgcs_handshake_initiate_batch's
HS_FINISHED = 6  # wgcs_handshake_finish_batch's
HS_START_COOKIE = 0x1  # wgcs_hs_start.flags: cookie[] is valid
HS_STATE_ZEROED, HS_STATE_INITIATED = 0, 1  # wgcs_hs_state.state
HS_ACCEPTED = 7  # wgcs_handshake_accept_batch's
HS_PEER_ZEROED, HS_PEER_CONSUMED = 0, 1  # wgcs_hs_peer.state
HS_PEER_SEEN, HS_PEER_COOKIE = 0x1, 0x2  # wgcs_hs_peer.flags: the peer has consumed before; cookie[] is valid
HS_BEGUN = 8  # wgcs_keypairs_begin_*_batch's
SESSION_NO_KEYPAIR = 0xFFFFFFFE  # a wgcs_session_slot key: the index is taken, its keypair is nil
KEYPAIR_SET, KEYPAIR_INITIATOR = 0x1, 0x2  # wgcs_keypair_ref.flags
HS_STARTED = 9  # wgcs_rekey_start_batch's
SESSION_EXPIRED = 0xFFFFFFFD  # a wgcs_aead_pkt key: the keypair is past RejectAfterTime
REJECT_AFTER_TIME_NS, REKEY_AFTER_TIME_NS = 180_000_000_000, 120_000_000_000  # constants.go:26, :15
REKEY_TIMEOUT_NS, KEEPALIVE_TIMEOUT_NS = 5_000_000_000, 10_000_000_000  # :18, :30
REKEY_LAST_MINUTE = 0x1  # wgcs_rekey.flags: timers.sentLastMinuteHandshake
(REKEY_WANT_NO_KEYPAIR, REKEY_WANT_REJECT_MESSAGES, REKEY_WANT_REJECT_TIME, REKEY_WANT_REKEY_MESSAGES,
 REKEY_WANT_REKEY_TIME, REKEY_WANT_LAST_MINUTE, REKEY_WANT_HOST) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40  # .want
REKEY_WANT_NEW_HANDSHAKE, REKEY_WANT_RETRY = 0x80, 0x100  # .want: expiredNewHandshake, expiredResendHandshake
(TIMER_NEW_HANDSHAKE, TIMER_RESEND_HANDSHAKE, TIMER_SEND_KEEPALIVE, TIMER_KEEPALIVE,
 TIMER_ZERO_OUT_KEYS) = range(5)  # wgcs_timers: bit i of pending, deadline_ns[i]
TIMERS_ACTIVE, TIMERS_NEED_ANOTHER, TIMERS_CLEAR_SRC, TIMERS_KEEPALIVE_NOW = 0x1, 0x2, 0x4, 0x8  # wgcs_timers.flags
TIMERS_JITTER_MAX_MS, TIMERS_MAX_ATTEMPTS = 334, 18  # constants.go:24, :19
TIMERS_ZERO_KEYS_NS = 3 * REJECT_AFTER_TIME_NS  # RejectAfterTime * 3
(TIMERS_ACT_KEEPALIVE, TIMERS_ACT_DEFERRED, TIMERS_ACT_FLUSH_STAGED, TIMERS_ACT_ZEROED,
 TIMERS_ACT_GAVE_UP) = 0x20, 0x40, 0x80, 0x100, 0x200  # wgcs_timers_expire_batch's d_actions; bits 0..4: timer i fired
RL_PACKET_COST_NS, RL_MAX_TOKENS_NS, RL_CLEANUP_NS = 50_000_000, 250_000_000, 1_000_000_000  # ratelimiter.go:14, :19, :21
RL_CLAIMED = 0x80000000  # wgcs_rl_entry.state inside a call: | the claiming row
HS_COOKIE_KEPT = 10  # wgcs_cookie_consume_batch's
COOKIE_GEN_HAS_MAC1 = 0x1  # wgcs_cookie_gen.flags: hasLastMAC1
COOKIE_REFRESH_NS = 120_000_000_000  # CookieRefreshTime, cookie.go:17
PEER_RUNNING = 0x1  # wgcs_peer_key.flags: peer.isRunning
GROUP_DATA = 0x1  # wgcs_write_group.flags: dataPacketReceived, receive.go:436
STAGED_RELEASED = 11  # wgcs_staged_release_batch's
STAGED_NONE, STAGED_EVICTED = 0xFFFFFFFF, 0xFFFFFFFE  # wgcs_staged_stage_batch's d_where: not staged; evicted in the call


class WgcsError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"wgcs error {code}: {msg}")
        self.code = code


class VirtioHdr(C.Structure):
    _fields_ = [
        ("flags", C.c_uint8), ("gso_type", C.c_uint8), ("hdr_len", C.c_uint16),
        ("gso_size", C.c_uint16), ("csum_start", C.c_uint16), ("csum_offset", C.c_uint16),
    ]


class AeadKey(C.Structure):  # wgcs_aead_key
    _fields_ = [("key", C.c_uint8 * 32), ("remote_index", C.c_uint32), ("pad", C.c_uint32 * 3)]


class AeadPkt(C.Structure):  # wgcs_aead_pkt
    _fields_ = [("off", C.c_uint64), ("counter", C.c_uint64), ("len", C.c_uint32), ("key", C.c_uint32)]


_lib = None


def declared_symbols() -> list[str]:
    """Function names declared in include/wgcsum.h."""
    with open(HEADER_PATH) as f:
        src = f.read()
    inline = set(re.findall(r"static inline [^(]*\b(wgcs_[a-z0-9_]+)\s*\(", src))  # header-only helpers
    return sorted(set(re.findall(r"\b(wgcs_[a-z0-9_]+)\s*\(", src)) - inline)


def load() -> C.CDLL:
    """Load libwgcsum.so.  If the process also uses torch, import torch FIRST:
    torch ships its own libamdhip64.so.7 and the dynamic linker then binds our
    library to that already-loaded runtime (one HIP runtime per process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, sz, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
    u8pp = C.POINTER(C.POINTER(C.c_uint8))
    sig = {
        "wgcs_abi_version": ([], i32),
        "wgcs_device_count": ([C.POINTER(i32)], i32),
        "wgcs_init": ([i32, C.POINTER(vp)], i32),
        "wgcs_destroy": ([vp], i32),
        "wgcs_strerror": ([i32], C.c_char_p),
        "wgcs_last_error": ([vp], C.c_char_p),
        "wgcs_sync": ([vp], i32),
        "wgcs_num_cu": ([vp], i32),
        "wgcs_checksum_batch": ([vp, i32, C.c_uint, vp, vp, vp, u32, vp, vp], i32),
        "wgcs_checksum_batches": ([vp, i32, C.c_uint, vp, u32, vp, u32, vp, vp], i32),
        "wgcs_gso_split_batch": ([vp, vp, vp, u32, vp, u32, u32, u32, vp, vp, vp, vp], i32),
        "wgcs_gso_kernel_shape": ([vp, vp, vp, vp], i32),
        "wgcs_handle_gro_batch": ([vp, vp, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_checksum": ([vp, vp, sz, u64, C.POINTER(C.c_uint16)], i32),
        "wgcs_checksum_valid": ([vp, vp, sz, C.c_uint8, C.c_uint8, i32, C.POINTER(i32)], i32),
        "wgcs_checksum_valid_cap": ([vp, vp, sz, sz, C.c_uint8, C.c_uint8, i32, C.POINTER(i32)], i32),
        "wgcs_gso_none_checksum": ([vp, vp, sz, C.c_uint16, C.c_uint16], i32),
        "wgcs_checksum_batch_host": ([vp, i32, C.c_uint, vp, sz, vp, vp, u32, vp], i32),
        "wgcs_gso_split": ([vp, vp, sz, C.POINTER(VirtioHdr), u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32, i32,
                            C.POINTER(i32)], i32),
        "wgcs_handle_virtio_read": ([vp, vp, sz, u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32, C.POINTER(i32)], i32),
        "wgcs_handle_virtio_read_cap": ([vp, vp, sz, sz, u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32,
                                         C.POINTER(i32)], i32),
        "wgcs_gso_split_cap": ([vp, vp, sz, sz, C.POINTER(VirtioHdr), u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32,
                                i32, C.POINTER(i32)], i32),
        "wgcs_handle_gro": ([vp, u8pp, C.POINTER(sz), C.POINTER(sz), i32, i32, i32, C.POINTER(i32), C.POINTER(i32)],
                            i32),
        "wgcs_stager_create": ([vp, u32, u32, sz, u32, u32, C.POINTER(vp)], i32),
        "wgcs_stager_destroy": ([vp], i32),
        "wgcs_stager_push": ([vp, vp, sz, C.POINTER(i32)], i32),
        "wgcs_stager_push_many": ([vp, C.POINTER(vp), C.POINTER(sz), i32, C.POINTER(i32), C.POINTER(i32)], i32),
        "wgcs_stager_reserve": ([vp, sz, C.POINTER(vp), C.POINTER(i32)], i32),
        "wgcs_stager_commit": ([vp, i32, sz], i32),
        "wgcs_stager_submit": ([vp, C.POINTER(u64)], i32),
        "wgcs_stager_wait": ([vp, u64], i32),
        "wgcs_stager_result": ([vp, u64, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp)], i32),
        "wgcs_get_gso_size": ([vp, sz, C.POINTER(i32)], i32),
        "wgcs_set_gso_size": ([vp, C.POINTER(sz), sz, C.c_uint16], i32),
        "wgcs_split_messages_batch": ([vp, vp, u64, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp], i32),
        "wgcs_coalesce_messages_batch": ([vp, vp, u64, u32, vp, vp, vp, u32, u32, i32, vp, vp, vp, vp, vp], i32),
        "wgcs_split_messages": ([vp, u8pp, sz, C.POINTER(i32), u8pp, C.POINTER(sz), i32, i32, C.POINTER(i32),
                                 C.POINTER(i32)], i32),
        "wgcs_coalesce_messages": ([vp, u8pp, C.POINTER(sz), C.POINTER(sz), i32, i32, vp, sz, u8pp, C.POINTER(sz),
                                    C.POINTER(sz), C.POINTER(i32), C.POINTER(sz), C.POINTER(i32)], i32),
        "wgcs_stager_copy_out": ([vp, u64, i32, u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32, C.POINTER(i32)], i32),
        "wgcs_wstager_create": ([vp, u32, u32, u32, sz, C.POINTER(vp)], i32),
        "wgcs_wstager_destroy": ([vp], i32),
        "wgcs_wstager_push": ([vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), i32, i32, i32, C.POINTER(i32)], i32),
        "wgcs_wstager_push_pinned": ([vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), i32, i32, i32,
                                      C.POINTER(i32)], i32),
        "wgcs_wstager_submit": ([vp, C.POINTER(u64)], i32),
        "wgcs_ring_create": ([vp, u32, C.POINTER(vp)], i32),
        "wgcs_ring_destroy": ([vp], i32),
        "wgcs_ring_info": ([vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)], i32),
        "wgcs_ring_checksum_valid": ([vp, vp, sz, C.c_uint8, C.c_uint8, i32, C.POINTER(i32)], i32),
        "wgcs_ring_checksum_valid_cap": ([vp, vp, sz, sz, C.c_uint8, C.c_uint8, i32, C.POINTER(i32)], i32),
        "wgcs_ring_handle_virtio_read": ([vp, vp, sz, u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32,
                                          C.POINTER(i32)], i32),
        "wgcs_ring_handle_virtio_read_cap": ([vp, vp, sz, sz, u8pp, C.POINTER(sz), i32, C.POINTER(i32), i32,
                                              C.POINTER(i32)], i32),
        "wgcs_host_alloc": ([vp, sz, C.POINTER(vp)], i32),
        "wgcs_host_free": ([vp, vp], i32),
        "wgcs_stream_wait_flag": ([vp, vp, vp, u32], i32),
        "wgcs_wstager_wait": ([vp, u64], i32),
        "wgcs_wstager_result": ([vp, u64, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(vp),
                                 C.POINTER(sz)], i32),
        "wgcs_padding": ([sz, u32], i32),
        "wgcs_aead_seal_batch": ([vp, vp, vp, vp, u32, u32, u32, vp, vp], i32),
        "wgcs_aead_open_batch": ([vp, vp, vp, vp, u32, u32, vp, vp, vp], i32),
        "wgcs_aead_seal": ([vp, vp, u32, u64, vp, sz, sz, u32, C.POINTER(sz)], i32),
        "wgcs_aead_open": ([vp, vp, vp, sz, C.POINTER(u64), C.POINTER(i32)], i32),
        "wgcs_router_create": ([], vp),
        "wgcs_router_destroy": ([vp], None),
        "wgcs_router_insert": ([vp, vp, sz, C.c_uint8, u32], i32),
        "wgcs_router_remove": ([vp, vp, sz, C.c_uint8, u32], i32),
        "wgcs_router_remove_by_peer": ([vp, u32], i32),
        "wgcs_router_find": ([vp, vp, sz], u32),
        "wgcs_router_peer_prefixes": ([vp, u32, vp, sz, C.POINTER(sz)], i32),
        "wgcs_router_image_size": ([vp], sz),
        "wgcs_router_write_image": ([vp, vp, sz, C.POINTER(sz)], i32),
        "wgcs_router_image_find": ([vp, sz, vp, sz, C.POINTER(u32)], i32),
        "wgcs_session_table_build": ([vp, vp, u32, vp, u32], i32),
        "wgcs_recv_classify_batch": ([vp, vp, vp, u64, vp, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_recv_source_batch": ([vp, vp, vp, vp, vp, u32, u32, vp, sz, vp, vp, vp], i32),
        "wgcs_route_dst_batch": ([vp, vp, vp, u64, u32, vp, u32, vp, sz, vp, vp], i32),
        "wgcs_replay_validate": ([vp, u64, u64], i32),
        "wgcs_replay_reset": ([vp], None),
        "wgcs_keyorder_work_bytes": ([u32], sz),
        "wgcs_replay_batch": ([vp, vp, vp, vp, u32, vp, u32, u64, vp, vp, sz, vp], i32),
        "wgcs_send_assign_batch": ([vp, vp, vp, vp, vp, u32, u32, u64, vp, u32, vp, u32, u64, vp, vp, vp, vp, sz, vp],
                                   i32),
        "wgcs_write_build_batch": ([vp, vp, vp, u32, u32, vp, u32, i32, u32, u32, u32, vp, vp, vp, vp, vp, vp], i32),
        "wgcs_write_build_host": ([vp, vp, u32, u32, vp, u32, i32, u32, u32, u32, vp, vp, vp, vp, vp], i32),
        "wgcs_cookie_checker_init": ([vp, vp], i32),
        "wgcs_cookie_check_mac1": ([vp, vp, sz], i32),
        "wgcs_cookie_check_mac2": ([vp, vp, sz, vp], i32),
        "wgcs_cookie_create_reply": ([vp, vp, sz, vp, vp, vp], i32),
        "wgcs_cookie_add_macs": ([vp, vp, vp, sz, vp], i32),
        "wgcs_cookie_consume_reply": ([vp, vp, vp, vp], i32),
        "wgcs_handshake_screen_batch": ([vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_x25519": ([vp, vp, vp], i32),
        "wgcs_noise_responder_init": ([vp, vp, vp], i32),
        "wgcs_peer_keys_build": ([vp, vp, vp, vp, u32, vp], i32),
        "wgcs_peer_keys_find": ([vp, u32, vp], i32),
        "wgcs_noise_consume_initiation": ([vp, vp, u32, vp, sz, vp], i32),
        "wgcs_noise_create_initiation": ([vp, vp, vp, vp, u32, vp, vp, vp], i32),
        "wgcs_x25519_batch": ([vp, vp, vp, u32, vp, vp, vp], i32),
        "wgcs_handshake_consume_batch": ([vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp], i32),
        "wgcs_noise_create_response": ([vp, vp, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_noise_consume_response": ([vp, vp, vp, vp, vp, u32, vp, sz, C.POINTER(u32), vp, vp], i32),
        "wgcs_handshake_respond_batch": ([vp, vp, u32, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_handshake_initiate_batch": ([vp, vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_handshake_finish_batch": ([vp, vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_handshake_initiate_host": ([vp, u32, vp, vp, u32, u32, vp, u32, vp, vp], i32),
        "wgcs_handshake_finish_host": ([vp, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp], i32),
        "wgcs_peer_rows_build": ([vp, u32, vp, u32], i32),
        "wgcs_handshake_accept_batch": ([vp, vp, vp, u32, C.c_int64, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_handshake_accept_host": ([vp, vp, u32, C.c_int64, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_keypairs_begin_responder_batch": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp, vp, u32, vp, u32, vp, vp, u32,
                                                 vp, vp, sz, vp], i32),
        "wgcs_keypairs_begin_initiator_batch": ([vp, vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32, vp, vp, u32,
                                                 vp, u32, vp, vp, u32, vp, vp, sz, vp], i32),
        "wgcs_keypairs_received_batch": ([vp, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp], i32),
        "wgcs_keypairs_begin_responder_host": ([vp, vp, u32, C.c_int64, vp, u32, vp, vp, u32, vp, u32, vp, vp, u32, vp],
                                               i32),
        "wgcs_keypairs_begin_initiator_host": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32, vp, vp, u32, vp,
                                                u32, vp, vp, u32, vp], i32),
        "wgcs_keypairs_received_host": ([vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp], i32),
        "wgcs_rekey_recv_gate_batch": ([vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32, vp], i32),
        "wgcs_rekey_send_gate_batch": ([vp, vp, vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp, u32, u64, vp, vp, vp],
                                       i32),
        "wgcs_rekey_sent_batch": ([vp, vp, vp, vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp, u32, u64, vp, vp], i32),
        "wgcs_rekey_received_batch": ([vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp, vp], i32),
        "wgcs_rekey_responded_batch": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp], i32),
        "wgcs_rekey_start_batch": ([vp, C.c_int64, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, sz, vp], i32),
        "wgcs_rekey_recv_gate_host": ([vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32], i32),
        "wgcs_rekey_send_gate_host": ([vp, vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp, u32, u64, vp, vp], i32),
        "wgcs_rekey_sent_host": ([vp, vp, vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp, u32, u64, vp], i32),
        "wgcs_rekey_received_host": ([vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp], i32),
        "wgcs_rekey_responded_host": ([vp, vp, u32, C.c_int64, vp, u32], i32),
        "wgcs_rekey_start_host": ([C.c_int64, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp], i32),
        "wgcs_timers_jitter_ms": ([u32, u32], u32),
        "wgcs_timers_sent_batch": ([vp, vp, vp, vp, vp, vp, u32, u32, C.c_int64, u32, vp, u32, vp, u32, vp], i32),
        "wgcs_timers_received_batch": ([vp, vp, u32, u32, C.c_int64, vp, u32, vp, u32, vp], i32),
        "wgcs_timers_initiated_batch": ([vp, vp, vp, vp, u32, C.c_int64, u32, vp, u32, vp], i32),
        "wgcs_timers_responded_batch": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp], i32),
        "wgcs_timers_finished_batch": ([vp, vp, vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, vp, u32, vp], i32),
        "wgcs_timers_rotated_batch": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, vp, u32, vp], i32),
        "wgcs_timers_expire_batch": ([vp, C.c_int64, vp, vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, vp, vp,
                                      vp, vp, vp, vp, vp, sz, vp], i32),
        "wgcs_timers_sent_host": ([vp, vp, vp, vp, vp, u32, u32, C.c_int64, u32, vp, u32, vp, u32], i32),
        "wgcs_timers_received_host": ([vp, u32, u32, C.c_int64, vp, u32, vp, u32], i32),
        "wgcs_timers_initiated_host": ([vp, vp, vp, u32, C.c_int64, u32, vp, u32], i32),
        "wgcs_timers_responded_host": ([vp, vp, u32, C.c_int64, vp, u32], i32),
        "wgcs_timers_finished_host": ([vp, vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, vp, u32], i32),
        "wgcs_timers_rotated_host": ([vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, vp, u32], i32),
        "wgcs_timers_expire_host": ([C.c_int64, vp, vp, vp, u32, vp, vp, vp, u32, vp, u32, vp, vp, u32, u32, vp, vp, vp,
                                     vp, vp, vp], i32),
        "wgcs_ratelimit_home_slot": ([vp, u32], u32),
        "wgcs_ratelimit_allow": ([vp, u32, vp, C.c_int64], i32),
        "wgcs_ratelimit_batch": ([vp, vp, vp, u32, vp, u32, C.c_int64, vp, vp, vp, sz, vp], i32),
        "wgcs_ratelimit_cleanup_batch": ([vp, vp, vp, u32, C.c_int64, vp, vp], i32),
        "wgcs_ratelimit_batch_host": ([vp, vp, u32, vp, u32, C.c_int64, vp, vp], i32),
        "wgcs_ratelimit_cleanup_host": ([vp, vp, u32, C.c_int64, vp], i32),
        "wgcs_cookie_gen_build": ([vp, u32, vp], i32),
        "wgcs_cookie_initiated_batch": ([vp, vp, vp, vp, u32, vp, u32, vp], i32),
        "wgcs_cookie_responded_batch": ([vp, vp, vp, vp, u32, vp, u32, vp], i32),
        "wgcs_cookie_consume_batch": ([vp, vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp,
                                       u32, vp, vp, vp], i32),
        "wgcs_cookie_age_batch": ([vp, C.c_int64, vp, vp, u32, vp], i32),
        "wgcs_cookie_initiated_host": ([vp, vp, vp, u32, vp, u32], i32),
        "wgcs_cookie_responded_host": ([vp, vp, vp, u32, vp, u32], i32),
        "wgcs_cookie_consume_host": ([vp, vp, vp, u32, C.c_int64, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, u32,
                                      vp, vp], i32),
        "wgcs_cookie_age_host": ([C.c_int64, vp, vp, u32], i32),
        "wgcs_staged_stage_batch": ([vp, vp, u64, vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, u32, u32,
                                     vp, vp, sz, vp], i32),
        "wgcs_staged_release_batch": ([vp, C.c_int64, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp, u32, u32, u64, u32, vp, vp,
                                       vp, vp, vp, vp, vp, vp, sz, vp], i32),
        "wgcs_staged_flush_batch": ([vp, vp, vp, vp, vp, u32, vp], i32),
        "wgcs_staged_stage_host": ([vp, u64, vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, u32, u32, vp,
                                    vp, sz], i32),
        "wgcs_staged_release_host": ([C.c_int64, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp, u32, u32, u64, u32, vp, vp, vp,
                                      vp, vp, vp, vp], i32),
        "wgcs_staged_flush_host": ([vp, vp, vp, vp, u32], i32),
        "wgcs_endpoint_recv_batch": ([vp, vp, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp], i32),
        "wgcs_endpoint_set_received_batch": ([vp, vp, u32, u32, vp, u32, vp, u32, vp, vp, vp, u32, vp], i32),
        "wgcs_endpoint_set_accepted_batch": ([vp, vp, u32, vp, u32, vp, vp, vp, u32, vp], i32),
        "wgcs_endpoint_set_finished_batch": ([vp, vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, u32, vp], i32),
        "wgcs_endpoint_dst_jobs_batch": ([vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp,
                                          vp], i32),
        "wgcs_endpoint_dst_initiated_batch": ([vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_endpoint_dst_responded_batch": ([vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_coalesce_messages_dst_batch": ([vp, vp, u64, u32, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp], i32),
        "wgcs_endpoint_recv_host": ([vp, vp, vp, vp, u32, vp, u32, u32, vp, vp], i32),
        "wgcs_endpoint_set_received_host": ([vp, u32, u32, vp, u32, vp, u32, vp, vp, vp, u32], i32),
        "wgcs_endpoint_set_accepted_host": ([vp, u32, vp, u32, vp, vp, vp, u32], i32),
        "wgcs_endpoint_set_finished_host": ([vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, u32], i32),
        "wgcs_endpoint_dst_jobs_host": ([vp, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp], i32),
        "wgcs_endpoint_dst_initiated_host": ([vp, vp, u32, vp, vp, u32, vp, vp, vp], i32),
        "wgcs_endpoint_dst_responded_host": ([vp, vp, u32, vp, vp, u32, vp, vp, vp], i32),
    }
    missing = [name for name in sig if not hasattr(L, name)]
    if missing:
        # only an explicit A/B build of an older revision may lack entry points
        # (scripts/probe_lib_bench.sh sets WGCS_LIB_PARTIAL=1); anything else
        # fails here, at load, not later at the first call
        if os.environ.get("WGCS_LIB_PARTIAL") != "1":
            raise RuntimeError(f"{LIB_PATH}: missing wgcsum entry points {missing} (a stale or mismatched library; "
                               "rebuild with `python -m wireguard_amd.build`)")
        import warnings

        warnings.warn(f"{LIB_PATH}: partial A/B library without {missing}", RuntimeWarning, stacklevel=2)
    for name, (args, res) in sig.items():
        if name in missing:
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L
