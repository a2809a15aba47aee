"""A sequential restatement of the stateful tail of ConsumeMessageInitiation
(device/noise.go:458-491) for a batch of consumed initiations, taken one after
another in row order under a clock that stands at `now`.

This is the oracle for wgcs_handshake_accept_host / wgcs_handshake_accept_batch.
It is written from the Go text, line by line, and knows nothing of claims,
winners or ranks: each row meets the Handshake its peer's earlier rows left.

  timestamp.After(hs.lastTimestamp)      bytes.Compare(t1[:], t2[:]) > 0, tai64n/tai64n.go:54
  time.Since(hs.lastInitiationConsumption) <= HandshakeInitationRate
                                         now - last <= time.Second / 50 (device/constants.go:33); a peer that
                                         never consumed holds the zero time.Time, ages ago: no flood
  replay is reported before flood        :461-472
  the update                             :474-488

The caller's side of CreateMessageResponse is a ticket per response, taken in
the order the reference would call sessions.NewIndex.  An initiation that would
be accepted when the tickets are spent is ERR_BATCH_FULL: the peer's row of the
state table stays as it was, so that the retry is accepted, while the later
rows of that peer in this batch are still judged against it.
"""
import numpy as np

from wireguard_amd.noise import HS_PEER_DTYPE, HS_RESP_DTYPE

HS_CONSUMED, HS_ACCEPTED = 3, 7
ERR_BATCH_FULL, ERR_REPLAY, ERR_NO_PEER, ERR_FLOOD = -14, -20, -23, -25
PEER_NONE = 0xFFFFFFFF
RATE_NS = 10**9 // 50  # HandshakeInitationRate
PEER_CONSUMED = 1      # handshakeInitiationConsumed
SEEN, COOKIE = 1, 2    # wgcs_hs_peer.flags


def after(t1: bytes, t2: bytes) -> bool:
    return t1 > t2  # bytes.Compare(t1[:], t2[:]) > 0


def accept(init, gate, now, table, peer_rows, peers, tickets):
    """(verdict, peers after the batch, the descriptor array, the count)."""
    n = len(init)
    verdict = np.zeros(n, np.int32)
    peers = np.array(peers, dtype=HS_PEER_DTYPE)
    resp = np.zeros(len(tickets), HS_RESP_DTYPE)
    resp["init_row"] = 0xFFFFFFFF
    handshake = {}  # table row -> [lastTimestamp, lastInitiationConsumption or None]: what the peer's next row meets
    used = 0
    for q in range(n):
        if gate[q] != HS_CONSUMED:
            verdict[q] = gate[q]
            continue
        peer = int(init["peer"][q])
        row = int(peer_rows[peer]) if peer < len(peer_rows) else PEER_NONE
        if row == PEER_NONE or row >= len(peers) or int(table["peer"][row]) != peer:
            verdict[q] = ERR_NO_PEER
            continue
        if row not in handshake:
            seen = int(peers["flags"][row]) & SEEN
            handshake[row] = [peers["last_timestamp"][row].tobytes(),
                              int(peers["last_consumption_ns"][row]) if seen else None]
        hs = handshake[row]
        timestamp = init["timestamp"][q].tobytes()
        replay = not after(timestamp, hs[0])                     # :458
        flood = hs[1] is not None and now - hs[1] <= RATE_NS     # :459
        if replay:                                               # :461
            verdict[q] = ERR_REPLAY
            continue
        if flood:                                                # :469
            verdict[q] = ERR_FLOOD
            continue
        if after(timestamp, hs[0]):                              # :480
            hs[0] = timestamp
        if hs[1] is None or now > hs[1]:                         # :484
            hs[1] = now
        if used == len(tickets):
            verdict[q] = ERR_BATCH_FULL
            continue
        j, used = used, used + 1
        flags = int(peers["flags"][row])
        peers["last_timestamp"][row] = np.frombuffer(hs[0], np.uint8)
        peers["last_consumption_ns"][row] = hs[1]
        peers["flags"][row] = flags | SEEN
        peers["remote_index"][row] = init["sender"][q]           # :477
        peers["state"][row] = PEER_CONSUMED                      # :487
        t = tickets[j]
        resp[j] = (q, row, t["local_index"], t["send_key"], t["recv_key"], 1 if flags & COOKIE else 0, 0,
                   t["ephemeral_private"], peers["cookie"][row] if flags & COOKIE else np.zeros(16, np.uint8))
        verdict[q] = HS_ACCEPTED
    return verdict, peers, resp, used
