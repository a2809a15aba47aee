"""A literal restatement of keypair rotation, device/noise.go:664-754 with
device/sessions.go and DeleteSession (device/keypair.go:64-68), as objects and
a dict.

This is the oracle for the wgcs_keypairs_*_host functions and, through them,
for the device batches.  It is written from the Go text, line by line, and
knows nothing of slots, probes, claims or key order: a Device holds a
`sessions` dict of index -> Session, every Peer three Keypair references, and a
batch is its rows taken one after another.

What the device form adds to the reference is restated here too, and marked:
  * the AEAD key rows and their key -> peer id column are tables of the
    library, so DeleteSession also erases both key rows (the reference cannot,
    keypair.go:12-17) and BeginSymmetricSession names the peer in both;
  * a begin whose index sessions.AddKeypair would not find, or would find
    with a keypair, is refused (WGCS_ERR_NO_HANDSHAKE) where the reference
    rotates regardless;
  * sessions.Delete leaves a tombstone: the slot arrays never lose a slot, so
    a deleted index reads as "taken, keypair nil" until the host rebuilds the
    table.

render() gives the state as the bytes of the tables of include/wgcsum.h, on
the slot layout the caller built.
"""
import numpy as np

from wireguard_amd.keypairs import KEYPAIRS_DTYPE
from wireguard_amd.transport import AEAD_KEY_DTYPE

HS_NONE, HS_RESPONDED, HS_FINISHED, HS_BEGUN = 0, 4, 6, 8
ERR_INVALID_ARG, ERR_PACKET_TOO_SHORT, ERR_NO_HANDSHAKE = -1, -8, -24
PEER_NONE = 0xFFFFFFFF
NO_KEYPAIR = 0xFFFFFFFE
SET, INITIATOR = 1, 2
CLAIM_NONE = 0xFFFFFFFF


class Keypair:
    def __init__(self, send_key, recv_key, local_index, is_initiator, created_at):
        self.send_key, self.recv_key, self.local_index = send_key, recv_key, local_index  # encrypt, decrypt, localIndex
        self.is_initiator, self.created_at = is_initiator, created_at


class Session:
    def __init__(self, peer, handshake=None, keypair=None):
        self.peer, self.handshake, self.keypair = peer, handshake, keypair


class Keypairs:
    def __init__(self):
        self.previous = self.current = self.next = None


class Peer:
    def __init__(self, device, ident, row):
        self.device, self.id, self.row, self.keypairs = device, ident, row, Keypairs()

    def begin_symmetric_session(self, local_index, send_key, recv_key, is_initiator, now):
        """noise.go:664-722, the keys being in rows send_key / recv_key already."""
        d = self.device
        # create AEAD instances
        keypair = Keypair(send_key, recv_key, local_index, is_initiator, now)    # :664-673
        d.key_peer[send_key] = d.key_peer[recv_key] = self.id                    # (device form)
        # remap index
        d.sessions_add_keypair(local_index, keypair)                             # :675
        # rotate key pairs
        keypairs = self.keypairs
        current, previous, next_ = keypairs.current, keypairs.previous, keypairs.next  # :681-683
        if is_initiator:                                                         # :700
            if next_ is not None:                                                # :703
                keypairs.next = None                                             # :705
                keypairs.previous = next_                                        # :706
                d.delete_session(current)                                        # :707
            else:
                keypairs.previous = current                                      # :710
            d.delete_session(previous)                                           # :712
            keypairs.current = keypair                                           # :713
        else:
            keypairs.next = keypair                                              # :717
            d.delete_session(next_)                                              # :718
            keypairs.previous = None                                             # :719
            d.delete_session(previous)                                           # :720

    def received_with_new_keypair(self, new) -> bool:
        """noise.go:725-754"""
        keypairs = self.keypairs
        if keypairs.next is not new:                                             # :731, :740
            return False
        previous = keypairs.previous                                             # :748
        keypairs.previous = keypairs.current                                     # :749
        self.device.delete_session(previous)                                     # :750
        keypairs.current = keypairs.next                                         # :751
        keypairs.next = None                                                     # :752
        return True


class Device:
    def __init__(self, table, peer_rows, keys, key_peer):
        """table: PEER_KEY_DTYPE rows; peer_rows: id -> row; keys, key_peer: the library's two key tables."""
        self.sessions = {}        # SessionMap.m
        self.tombstones = set()   # (device form) indices sessions.Delete removed: their slots stay
        self.peers = [Peer(self, int(table["peer"][r]), r) for r in range(len(table))]
        self.peer_rows = np.array(peer_rows, dtype=np.uint32)
        self.keys = np.array(keys, dtype=AEAD_KEY_DTYPE)
        self.key_peer = np.array(key_peer, dtype=np.uint32)

    # ---- sessions.go
    def sessions_new_index(self, index, peer):                                   # :38-68, the index being the caller's
        self.sessions[index] = Session(peer, handshake=True)
        self.tombstones.discard(index)

    def sessions_add_keypair(self, index, keypair):                              # :71-82
        session = self.sessions.get(index)
        if session is None:
            if index not in self.tombstones:
                return
            self.tombstones.discard(index)                                       # (device form) the slot is there
            session = Session(None)
        self.sessions[index] = Session(session.peer, keypair=keypair)

    def delete_session(self, key):                                               # keypair.go:64-68
        if key is not None:
            if self.sessions.pop(key.local_index, None) is not None:             # sessions.go:32-36
                self.tombstones.add(key.local_index)
            for row in (key.send_key, key.recv_key):                             # (device form)
                self.keys[row:row + 1].view(np.uint8)[:] = 0
                self.key_peer[row] = PEER_NONE

    # ---- one descriptor of a begin batch, with the device form's checks in front
    def begin(self, peer_row, local_index, send_key, recv_key, is_initiator, now) -> int:
        n_keys = len(self.keys)
        if peer_row >= len(self.peers) or send_key >= n_keys or recv_key >= n_keys or send_key == recv_key:
            return ERR_INVALID_ARG
        session = self.sessions.get(local_index)
        taken_without_keypair = (session is not None and session.keypair is None) or local_index in self.tombstones
        if not taken_without_keypair:                                            # (device form) DESIGN 8
            return ERR_NO_HANDSHAKE
        self.peers[peer_row].begin_symmetric_session(local_index, send_key, recv_key, is_initiator, now)
        return HS_BEGUN

    def begin_responder(self, resp, gate, now):
        status = np.zeros(len(resp), np.int32)
        for j in range(len(resp)):
            if gate[j] != HS_RESPONDED:
                status[j] = HS_NONE
                continue
            r = resp[j]
            status[j] = self.begin(int(r["peer_row"]), int(r["local_index"]), int(r["send_key"]), int(r["recv_key"]),
                                   False, now)
        return status

    def begin_initiator(self, arena, pkts, gate, now, hs_index, states):
        """hs_index: dict local index -> row of states, the handshakes finish found in flight."""
        status = np.zeros(len(pkts), np.int32)
        for q in range(len(pkts)):
            if gate[q] != HS_FINISHED:
                status[q] = HS_NONE
                continue
            off = int(pkts["off"][q])
            receiver = int.from_bytes(arena[off + 8:off + 12].tobytes(), "little")   # msg.Receiver
            row = hs_index.get(receiver)
            if row is None or row >= len(states) or int(states["local_index"][row]) != receiver:
                status[q] = ERR_NO_HANDSHAKE
                continue
            st = states[row]
            status[q] = self.begin(int(st["peer_row"]), receiver, int(st["send_key"]), int(st["recv_key"]), True, now)
        return status

    # ---- receive.go:414-429 for the rows of one batch, in turn
    def received(self, pkts, verdict):
        rotated = np.zeros(len(pkts), np.uint32)
        for i in range(len(pkts)):
            key, v = int(pkts["key"][i]), int(verdict[i])
            if key >= len(self.keys) or (v < 0 and v != ERR_PACKET_TOO_SHORT):
                continue                                                         # never reached :422
            ident = int(self.key_peer[key])
            row = int(self.peer_rows[ident]) if ident < len(self.peer_rows) else PEER_NONE
            if row == PEER_NONE or row >= len(self.peers):
                continue
            peer = self.peers[row]
            k = peer.keypairs
            elem_keypair = next((x for x in (k.next, k.current, k.previous) if x is not None and x.recv_key == key), None)
            if elem_keypair is not None and peer.received_with_new_keypair(elem_keypair):   # :422
                rotated[i] = 1
        return rotated

    # ---- the state as the library's tables
    def render(self, slots_layout, peer_keys_layout):
        """(kp, slots, peer_keys, keys, key_peer): slots_layout / peer_keys_layout are the arrays the host built,
        of which only the occupied slots' indices are taken."""
        kp = np.zeros(len(self.peers), KEYPAIRS_DTYPE)
        kp["claim"] = CLAIM_NONE
        for p in self.peers:
            for name in ("previous", "current", "next"):
                x = getattr(p.keypairs, name)
                if x is not None:
                    kp[name][p.row] = (x.send_key, x.recv_key, x.local_index, SET | (INITIATOR if x.is_initiator else 0),
                                       x.created_at)
        slots = np.array(slots_layout)
        for s in slots:
            if s["key"] != 0xFFFFFFFF:
                session = self.sessions.get(int(s["index"]))
                s["key"] = NO_KEYPAIR if session is None or session.keypair is None else session.keypair.recv_key
        by_id = {p.id: p for p in self.peers}
        peer_keys = np.array(peer_keys_layout)
        for s in peer_keys:
            if s["key"] != 0xFFFFFFFF:
                p = by_id.get(int(s["index"]))
                if p is not None:   # an id without a peer row keeps what the host wrote
                    s["key"] = NO_KEYPAIR if p.keypairs.current is None else p.keypairs.current.send_key
        return kp, slots, peer_keys, self.keys.copy(), self.key_peer.copy()
