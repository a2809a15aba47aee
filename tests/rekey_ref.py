"""A literal restatement of the reference's keypair expiry and rekey rules, as
plain Python over objects (test infrastructure; never on a hot path):

  Device.recv_gate    RoutineReceiveIncoming's keypair lookup and expiry check     device/receive.go:162-170
  Device.send_gate    the head of SendStagedPackets                                device/send.go:368-374
  Device.sent         keepKeyFreshSending (send.go:213-227, called at :523), and the goto top of :419-420
                      that brings a job whose nonces ran out back to :370
  Device.received     keepKeyFreshReceiving                                        receive.go:80-91, :486-488
  Device.responded    SendHandshakeResponse's lastSentHandshake                    send.go:131-133
  Device.start        SendHandshakeInitiation up to CreateMessageInitiation        send.go:84-100

A Device holds a dict of Peer objects by peer id; a Peer holds its three
Keypair objects (or None), handshake.lastSentHandshake, the
sentLastMinuteHandshake timer flag and the set of reasons for which
SendHandshakeInitiation was asked for and has not run yet.  The clock is fixed
per call: time.Now() and time.Since() read Device.now.  render() gives the
state as the bytes of the wgcs_rekey table.
"""
import numpy as np

from wireguard_amd.noise import HS_START_DTYPE
from wireguard_amd.rekey import REKEY_DTYPE

SECOND = 1_000_000_000
RekeyAfterMessages = 1 << 60            # constants.go:12
RejectAfterMessages = (1 << 64) - (1 << 13) - 1  # :14
RekeyAfterTime = 120 * SECOND           # :15
RekeyTimeout = 5 * SECOND               # :18
RejectAfterTime = 180 * SECOND          # :26
KeepaliveTimeout = 10 * SECOND          # :30

PEER_NONE = 0xFFFFFFFF
SESSION_EXPIRED = 0xFFFFFFFD
NO_KEY = 0xFFFFFFFF                     # send-assign's d_job_key of a dropped job
ERR_BATCH_FULL, ERR_KEY_EXPIRED, ERR_REKEY_TIMEOUT = -14, -26, -27
HS_NONE, HS_RESPONDED, HS_STARTED = 0, 4, 9
SET, INITIATOR = 1, 2                   # wgcs_keypair_ref.flags
HS_PEER_COOKIE, HS_START_COOKIE = 2, 1
LAST_MINUTE = 1                         # wgcs_rekey.flags
(WANT_NO_KEYPAIR, WANT_REJECT_MESSAGES, WANT_REJECT_TIME, WANT_REKEY_MESSAGES, WANT_REKEY_TIME, WANT_LAST_MINUTE,
 WANT_HOST) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40


class Keypair:
    def __init__(self, ref):
        self.send_key, self.recv_key = int(ref["send_key"]), int(ref["recv_key"])
        self.isInitiator = bool(int(ref["flags"]) & INITIATOR)
        self.createdAt = int(ref["created_ns"])


class Peer:
    def __init__(self, row, rekey_row, hs_peer_row):
        self.row = row
        self.current = self.previous = self.next = None
        self.lastSentHandshake = int(rekey_row["last_sent_ns"])
        self.sentLastMinuteHandshake = bool(int(rekey_row["flags"]) & LAST_MINUTE)
        self.want = int(rekey_row["want"])
        self.other_flags = int(rekey_row["flags"]) & ~LAST_MINUTE
        self.cookie = bytes(hs_peer_row["cookie"]) if int(hs_peer_row["flags"]) & HS_PEER_COOKIE else None


class Device:
    def __init__(self, peer_rows, n_peers, rekey, hs_peers, key_peer):
        """peer_rows: id -> row (wgcs_peer_rows_build); rekey, hs_peers: the tables as they stand"""
        self.peers, self.by_row = {}, [None] * n_peers
        for ident, row in enumerate(np.asarray(peer_rows).tolist()):
            if row != PEER_NONE and row < n_peers:
                self.peers[ident] = self.by_row[row] = Peer(row, rekey[row], hs_peers[row])
        self.key_peer = key_peer
        self.now = 0

    # the state the other sections own: the wgcs_keypairs rows and the key -> peer id column
    def load_keypairs(self, kp, key_peer):
        self.key_peer = key_peer
        for p in self.by_row:
            for name in ("current", "previous", "next"):
                ref = kp[name][p.row]
                setattr(p, name, Keypair(ref) if int(ref["flags"]) & SET else None)

    def since(self, t):  # time.Since
        return self.now - t

    def send_handshake_initiation(self, peer, reason):
        """peer.SendHandshakeInitiation(false) as the caller sees it: the request, which start() carries out"""
        peer.want |= reason

    # receive.go:162-170
    def recv_gate(self, keys, now):
        """keys: d_pkts[i].key as classify left it (sessions.Get found the key row) -> the keys afterwards"""
        self.now = now
        out = []
        for key in keys:
            out.append(key)
            peer = self.peers.get(int(self.key_peer[key])) if key < len(self.key_peer) else None
            if peer is None:
                continue
            keypair = next((k for k in (peer.current, peer.previous, peer.next) if k is not None and k.recv_key == key),
                           None)
            if keypair is None:  # :164-166
                continue
            if keypair.createdAt + RejectAfterTime < self.now:  # :168 createdAt.Add(RejectAfterTime).Before(time.Now())
                out[-1] = SESSION_EXPIRED
        return out

    def job_peer(self, j, peer, count, status, max_segs):
        if status[j] != 0 or not 1 <= count[j] <= max_segs:
            return None
        return self.peers.get(int(peer[j * max_segs]))

    # send.go:368-374
    def send_gate(self, peer, count, status_in, max_segs, now, send_nonce, limit):
        self.now = now
        out = []
        for j in range(len(count)):
            out.append(int(status_in[j]))
            p = self.job_peer(j, peer, count, status_in, max_segs)
            if p is None:
                continue
            keypair = p.current
            if keypair is not None and keypair.send_key >= len(send_nonce):
                continue  # no nonce to load: the job is send-assign's
            reason = 0
            if keypair is None:
                reason = WANT_NO_KEYPAIR                                # :369
            else:
                if int(send_nonce[keypair.send_key]) >= limit:
                    reason |= WANT_REJECT_MESSAGES                      # :370
                if self.since(keypair.createdAt) >= RejectAfterTime:
                    reason |= WANT_REJECT_TIME                          # :371
            if reason:
                self.send_handshake_initiation(p, reason)               # :372
                out[-1] = ERR_KEY_EXPIRED                               # :373 return: the packets stay staged
        return out

    # send.go:213-227 for a job that was sent, :419-420 -> :370 for one whose nonces ran out
    def sent(self, peer, count, status, job_key, max_segs, now, send_nonce, limit):
        self.now = now
        for j in range(len(count)):
            p = self.job_peer(j, peer, count, status, max_segs)
            if p is None:
                continue
            keypair = p.current
            if keypair is None:                                         # :215-217
                continue
            nonce = int(send_nonce[keypair.send_key]) if keypair.send_key < len(send_nonce) else None
            if int(job_key[j]) != NO_KEY:
                if nonce is not None and nonce > RekeyAfterMessages:    # :223
                    self.send_handshake_initiation(p, WANT_REKEY_MESSAGES)
                if keypair.isInitiator and self.since(keypair.createdAt) > RekeyAfterTime:  # :224
                    self.send_handshake_initiation(p, WANT_REKEY_TIME)
            elif nonce is not None and nonce >= limit:                  # :385-390, :419-420, :370
                self.send_handshake_initiation(p, WANT_REJECT_MESSAGES)

    # receive.go:80-91, called at :486-488 when validTailPacket is set
    def received(self, groups, now):
        self.now = now
        for g in groups:
            if int(g["tail"]) < 0:
                continue
            peer = self.peers.get(int(g["peer"]))
            if peer is None:
                continue
            if peer.sentLastMinuteHandshake:                            # :81-83
                continue
            keypair = peer.current
            if (keypair is not None and keypair.isInitiator and
                    self.since(keypair.createdAt) > RejectAfterTime - KeepaliveTimeout - RekeyTimeout):  # :85-87
                peer.sentLastMinuteHandshake = True                     # :88
                self.send_handshake_initiation(peer, WANT_LAST_MINUTE)  # :89

    # send.go:131-133
    def responded(self, resp, gate, now):
        self.now = now
        for j in range(len(gate)):
            if int(gate[j]) != HS_RESPONDED:
                continue
            row = int(resp["peer_row"][j])
            if row < len(self.by_row):
                self.by_row[row].lastSentHandshake = self.now

    # send.go:84-100 for every peer that was asked to, in row order (the order of NewIndex)
    def start(self, now, tickets):
        self.now = now
        n, n_tickets = len(self.by_row), len(tickets)
        status, reasons = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        start = np.zeros(n_tickets, HS_START_DTYPE)
        start["state_row"] = 0xFFFFFFFF
        start_peer = np.full(n_tickets, PEER_NONE, np.uint32)
        k = 0
        for peer in self.by_row:
            reasons[peer.row] = peer.want
            if not peer.want:
                status[peer.row] = HS_NONE
                continue
            if self.since(peer.lastSentHandshake) < RekeyTimeout:       # :89-92, :95-98
                peer.want = 0
                status[peer.row] = ERR_REKEY_TIMEOUT
                continue
            if k >= n_tickets:  # the caller paid for no more: the request waits
                status[peer.row] = ERR_BATCH_FULL
                k += 1
                continue
            peer.lastSentHandshake = self.now                           # :99
            peer.want = 0
            t, d = tickets[k], start[k]
            for f in ("state_row", "local_index", "send_key", "recv_key", "timestamp", "ephemeral_private"):
                d[f] = t[f]
            d["peer_row"] = peer.row
            if peer.cookie is not None:                                 # cookie.go:287-314: AddMACs writes MAC2
                d["flags"], d["cookie"] = HS_START_COOKIE, np.frombuffer(peer.cookie, np.uint8)
            start_peer[k] = peer.row
            status[peer.row] = HS_STARTED
            k += 1
        return dict(status=status, reasons=reasons, start=start, start_peer=start_peer,
                    count=np.array([min(k, n_tickets)], np.uint32))

    def render(self):
        out = np.zeros(len(self.by_row), REKEY_DTYPE)
        for p in self.by_row:
            out[p.row] = (p.lastSentHandshake, p.want, p.other_flags | (LAST_MINUTE if p.sentLastMinuteHandshake else 0))
        return out
