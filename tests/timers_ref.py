"""A literal restatement of the reference's peer timers, as plain Python over
objects (test infrastructure; never on a hot path):

  Timer                       Mod, Del, IsPending and NewTimer's callback      device/timers.go:11-71
  expired*                    the five expiry functions                        timers.go:73-144
  Peer.timers*                the hooks                                        timers.go:168-295
  Peer.SendKeepalive          device/send.go:193-209
  Peer.ZeroAndFlushAll        device/peer.go:241-260
  Device.sent                 RoutineSendToPeer's tail                         send.go:498-510
  Device.received             RoutineSendToInternet's tail                     device/receive.go:486-494
  Device.initiated            SendHandshakeInitiation                          send.go:85-87, :117-126
  Device.responded            RoutineHandshake and SendHandshakeResponse       receive.go:311-312, send.go:158-160
  Device.finished             RoutineHandshake                                 receive.go:339-348
  Device.rotated              RoutineSendToInternet                            receive.go:422-427
  Device.expire               every timer whose time has come, earliest first

A Device holds a dict of Peer objects by peer id; a Peer holds its five Timer
objects, handshakeAttempts, needAnotherKeepalive, keepaliveInterval,
lastHandshake and isRunning.  The clock is fixed per call: time.Now() reads
Device.now, and a Timer remembers the instant it was last set for.  The
keypairs, the sessions and the key rows are a keypairs_ref.Device; the words of
the wgcs_rekey table (the wishes for a handshake and sentLastMinuteHandshake)
belong to tests/rekey_ref.py and are passed in and out of a call as the table.

What the device form adds to the reference is restated here too, and marked:
  * rand.Int64N(RekeyTimeoutJitterMaxMs) is jitter_ms(seed, row), a fixed mix;
  * SendHandshakeInitiation leaves a wish that wgcs_rekey_start_batch carries
    out, so its `!isRetry` store (send.go:85-87) runs in Device.initiated, from
    the wishes start recorded;
  * SendKeepalive owes one keepalive job per peer and call, emitted in row
    order while there is room and deferred past it;
  * FlushStagedPackets, handshake.Clear and the endpoint are the host's: they
    leave an action bit or a flag.

render() gives the state as the bytes of the wgcs_timers table.
"""
import numpy as np

from wireguard_amd.timers import TIMERS_DTYPE

SECOND, MILLISECOND = 1_000_000_000, 1_000_000
RekeyTimeout = 5 * SECOND               # constants.go:18
MaxHandshakeAttempts = 90 // 5          # :19 uint32(RekeyAttemptTime / RekeyTimeout)
RekeyTimeoutJitterMaxMs = 334           # :24
RejectAfterTime = 180 * SECOND          # :26
KeepaliveTimeout = 10 * SECOND          # :30

PEER_NONE = 0xFFFFFFFF
NO_KEY = 0xFFFFFFFF                     # send-assign's d_job_key of a dropped job
HS_RESPONDED, HS_INITIATED, HS_FINISHED, HS_BEGUN = 4, 5, 6, 8
GROUP_DATA = 1                          # wgcs_write_group.flags
LAST_MINUTE = 1                         # wgcs_rekey.flags
WANT_NEW_HANDSHAKE, WANT_RETRY = 0x80, 0x100
ACTIVE, NEED_ANOTHER, CLEAR_SRC, KEEPALIVE_NOW = 1, 2, 4, 8    # wgcs_timers.flags
(ACT_KEEPALIVE, ACT_DEFERRED, ACT_FLUSH_STAGED, ACT_ZEROED, ACT_GAVE_UP) = 0x20, 0x40, 0x80, 0x100, 0x200
NAMES = ("newHandshake", "resendHandshake", "sendKeepalive", "keepalive", "zeroOutKeys")  # bit i, deadline_ns[i]


def fired(i):
    return 1 << i                       # WGCS_TIMERS_ACT_FIRED(i)


def jitter_ms(seed, row):
    """(device form) wgcs_timers_jitter_ms: rand.Int64N(RekeyTimeoutJitterMaxMs) from the call's seed and the row"""
    m = 0xFFFFFFFF
    x = (seed ^ (row * 0x9E3779B9)) & m
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return (x * RekeyTimeoutJitterMaxMs) >> 32


class Timer:
    """timers.go:11-71 over a clock that stands still during a call"""

    def __init__(self, peer, expFunc, isPending, when):
        self.peer, self.expFunc, self.isPending, self.when = peer, expFunc, isPending, when

    def Mod(self, d):                   # :42-47
        self.isPending = True
        self.when = self.peer.device.now + d        # t.Reset(d)

    def Del(self):                      # :49-54
        self.isPending = False

    def IsPending(self):                # :67-71
        return self.isPending

    def callback(self):                 # :26-37
        if not self.isPending:
            return
        self.isPending = False
        self.expFunc(self.peer)


def expiredNewHandshake(peer):          # :73-82
    peer.acted |= fired(0)
    peer.markEndpointSrcForClearing()
    peer.SendHandshakeInitiation(False)


def expiredResendHandshake(peer):       # :84-115
    peer.acted |= fired(1)
    if peer.handshakeAttempts > MaxHandshakeAttempts:
        peer.acted |= ACT_GAVE_UP
        if peer.timersActive():
            peer.sendKeepalive.Del()
        peer.FlushStagedPackets()
        if peer.timersActive() and not peer.zeroOutKeys.IsPending():
            peer.zeroOutKeys.Mod(RejectAfterTime * 3)
    else:
        peer.handshakeAttempts += 1
        peer.markEndpointSrcForClearing()
        peer.SendHandshakeInitiation(True)


def expiredSendKeepalive(peer):         # :119-127
    peer.acted |= fired(2)
    peer.SendKeepalive()
    if peer.needAnotherKeepalive:
        peer.needAnotherKeepalive = False
        if peer.timersActive():
            peer.sendKeepalive.Mod(KeepaliveTimeout)


def expiredKeepalive(peer):             # :131-135
    peer.acted |= fired(3)
    if peer.keepaliveInterval > 0:
        peer.SendKeepalive()


def expiredZeroOutKeys(peer):           # :137-144
    peer.acted |= fired(4)
    peer.ZeroAndFlushAll()


EXPIRED = (expiredNewHandshake, expiredResendHandshake, expiredSendKeepalive, expiredKeepalive, expiredZeroOutKeys)


class Peer:
    def __init__(self, device, row, t):
        self.device, self.row = device, row
        for i, name in enumerate(NAMES):            # timersInit, :146-152
            setattr(self, name, Timer(self, EXPIRED[i], bool(int(t["pending"]) >> i & 1), int(t["deadline_ns"][i])))
        flags = int(t["flags"])
        self.isRunning = bool(flags & ACTIVE)
        self.needAnotherKeepalive = bool(flags & NEED_ANOTHER)
        self.clearSrc, self.keepaliveNow = bool(flags & CLEAR_SRC), bool(flags & KEEPALIVE_NOW)
        self.other_flags = flags & ~(ACTIVE | NEED_ANOTHER | CLEAR_SRC | KEEPALIVE_NOW)
        self.other_pending = int(t["pending"]) & ~31
        self.handshakeAttempts, self.keepaliveInterval = int(t["attempts"]), int(t["keepalive_interval_s"])
        self.lastHandshake = int(t["last_handshake_ns"])
        self.want, self.sentLastMinuteHandshake = 0, False      # the wgcs_rekey row, loaded per call
        self.acted, self.staged, self.queued = 0, False, False  # one expire call's

    def timers(self):
        return [getattr(self, name) for name in NAMES]

    def timersActive(self):             # :168-170
        return self.isRunning

    def timersDataSent(self):           # :189-221
        if self.timersActive() and not self.newHandshake.IsPending():
            d = KeepaliveTimeout + RekeyTimeout + MILLISECOND * jitter_ms(self.device.jitter_seed, self.row)
            self.newHandshake.Mod(d)

    def timersAuthenticatedPacketReceived(self):    # :226-230
        if self.timersActive():
            self.newHandshake.Del()

    def timersDataReceived(self):       # :235-244
        if self.timersActive():
            if not self.sendKeepalive.IsPending():
                self.sendKeepalive.Mod(KeepaliveTimeout)
            else:
                self.needAnotherKeepalive = True

    def timersAuthenticatedPacketSent(self):        # :249-253
        if self.timersActive():
            self.sendKeepalive.Del()

    def timersAuthenticatedPacketTraversal(self):   # :259-264
        keepalive = self.keepaliveInterval
        if keepalive > 0 and self.timersActive():
            self.keepalive.Mod(keepalive * SECOND)

    def timersHandshakeInitiated(self):             # :268-274
        if self.timersActive():
            d = RekeyTimeout + MILLISECOND * jitter_ms(self.device.jitter_seed, self.row)
            self.resendHandshake.Mod(d)

    def timersHandshakeComplete(self):              # :279-286
        if self.timersActive():
            self.resendHandshake.Del()
        self.handshakeAttempts = 0
        self.sentLastMinuteHandshake = False
        self.lastHandshake = self.device.now

    def timersSessionDerived(self):                 # :291-295
        if self.timersActive():
            self.zeroOutKeys.Mod(RejectAfterTime * 3)

    def markEndpointSrcForClearing(self):           # (device form) the endpoint is the host's
        self.clearSrc = True

    def SendHandshakeInitiation(self, isRetry):     # (device form) send.go:84: the wish; start carries it out
        self.want |= WANT_RETRY if isRetry else WANT_NEW_HANDSHAKE

    def SendKeepalive(self):                        # send.go:193-209
        if not self.staged and self.isRunning:      # :194
            self.queued = True                      # (device form) :195-207, one per peer and call
        # :208 SendStagedPackets is the caller's next send batch

    def FlushStagedPackets(self):                   # (device form) the staged queue is the host's
        self.acted |= ACT_FLUSH_STAGED

    def ZeroAndFlushAll(self):                      # peer.go:241-260
        kd = self.device.kd
        keypairs = kd.peers[self.row].keypairs
        kd.delete_session(keypairs.current)         # :246
        kd.delete_session(keypairs.previous)        # :247
        kd.delete_session(keypairs.next)            # :248
        keypairs.current = None                     # :249
        keypairs.previous = None                    # :250
        keypairs.next = None                        # :251
        self.acted |= ACT_ZEROED                    # (device form) :254-258 are the host's
        self.FlushStagedPackets()                   # :259


class Device:
    def __init__(self, peer_rows, timers, kd=None):
        """peer_rows: id -> row (wgcs_peer_rows_build); timers: the table as it stands; kd: a keypairs_ref.Device"""
        n_peers = len(timers)
        self.peers, self.by_row, self.kd = {}, [Peer(self, r, timers[r]) for r in range(n_peers)], kd
        for ident, row in enumerate(np.asarray(peer_rows).tolist()):
            if row != PEER_NONE and row < n_peers:
                self.peers[ident] = self.by_row[row]
        self.now, self.jitter_seed = 0, 0

    # the words the rekey section owns
    def load_rekey(self, rekey):
        for p in self.by_row:
            p.want, p.sentLastMinuteHandshake = int(rekey["want"][p.row]), bool(int(rekey["flags"][p.row]) & LAST_MINUTE)

    def store_rekey(self, rekey):
        for p in self.by_row:
            rekey["want"][p.row] = p.want
            rekey["flags"][p.row] = (int(rekey["flags"][p.row]) & ~LAST_MINUTE) | (LAST_MINUTE if p.sentLastMinuteHandshake else 0)

    # send.go:498-510 for the jobs send-assign kept
    def sent(self, sizes, peer, count, status, job_key, max_segs, now, seed):
        self.now, self.jitter_seed = now, seed
        for j in range(len(count)):
            if int(job_key[j]) == NO_KEY or status[j] != 0 or not 1 <= count[j] <= max_segs:
                continue
            p = self.peers.get(int(peer[j * max_segs]))
            if p is None:
                continue
            dataSent = False                                            # :498
            for k in range(int(count[j])):
                if int(sizes[j * max_segs + k]) != 0:                   # :500 len(item.packet) != MessageKeepaliveSize
                    dataSent = True
            p.timersAuthenticatedPacketTraversal()                      # :505
            p.timersAuthenticatedPacketSent()                           # :506
            if dataSent:                                                # :508
                p.timersDataSent()

    # receive.go:486-494 for every group of the write builder
    def received(self, groups, now):
        self.now = now
        for g in groups:
            if int(g["tail"]) < 0:                                      # :486
                continue
            p = self.peers.get(int(g["peer"]))
            if p is None:
                continue
            p.timersAuthenticatedPacketTraversal()                      # :489
            p.timersAuthenticatedPacketReceived()                       # :490
            if int(g["flags"]) & GROUP_DATA:                            # :492
                p.timersDataReceived()

    # send.go:85-87 from the wishes start recorded, then :117-126 for the messages initiate built
    def initiated(self, reasons, start_peer, init_status, now, seed):
        self.now, self.jitter_seed = now, seed
        for p in self.by_row:
            if int(reasons[p.row]) & ~WANT_RETRY:                       # :85 !isRetry
                p.handshakeAttempts = 0
        for k in range(len(start_peer)):
            row = int(start_peer[k])
            if row >= len(self.by_row) or int(init_status[k]) != HS_INITIATED:
                continue
            p = self.by_row[row]
            p.timersAuthenticatedPacketTraversal()                      # :117
            p.timersAuthenticatedPacketSent()                           # :118
            p.timersHandshakeInitiated()                                # :126

    # receive.go:311-312 and send.go:158-160 for the descriptors respond answered
    def responded(self, resp, gate, now):
        self.now = now
        for j in range(len(gate)):
            if int(gate[j]) != HS_RESPONDED:                            # (device form) a refused one runs neither
                continue
            row = int(resp["peer_row"][j])
            if row >= len(self.by_row):
                continue
            p = self.by_row[row]
            p.timersAuthenticatedPacketTraversal()                      # receive.go:311
            p.timersAuthenticatedPacketReceived()                       # :312
            p.timersSessionDerived()                                    # send.go:158
            p.timersAuthenticatedPacketTraversal()                      # :159
            p.timersAuthenticatedPacketSent()                           # :160

    # receive.go:339-348 for the responses whose keypair begin installed
    def finished(self, arena, pkts, gate, begun, now, hs_index, states):
        self.now = now
        for q in range(len(pkts)):
            if int(begun[q]) != HS_BEGUN or int(gate[q]) != HS_FINISHED:        # :342-345
                continue
            off = int(pkts["off"][q])
            receiver = int.from_bytes(arena[off + 8:off + 12].tobytes(), "little")
            row = hs_index.get(receiver)
            if row is None or row >= len(states) or int(states["local_index"][row]) != receiver:
                continue
            row = int(states["peer_row"][row])
            if row >= len(self.by_row):
                continue
            p = self.by_row[row]
            p.timersAuthenticatedPacketTraversal()                      # :339
            p.timersAuthenticatedPacketReceived()                       # :340
            p.timersSessionDerived()                                    # :346
            p.timersHandshakeComplete()                                 # :347
            p.keepaliveNow = True                                       # :348 (device form) the expire call sends it

    # receive.go:422-427 for the rows that promoted a keypair
    def rotated(self, pkts, rotated, now, key_peer):
        self.now = now
        for i in range(len(pkts)):
            key = int(pkts["key"][i])
            if int(rotated[i]) != 1 or key >= len(key_peer):
                continue
            p = self.peers.get(int(key_peer[key]))
            if p is not None:
                p.timersHandshakeComplete()                             # :426

    # every timer whose time has come, earliest first; then the keepalives that are owed, in row order
    def expire(self, now, staged, n_ka_max):
        self.now = now
        n = len(self.by_row)
        actions = np.zeros(n, np.uint32)
        jobs = []
        for p in self.by_row:
            p.acted, p.queued = 0, False
            p.staged = staged is not None and int(staged[p.row]) != 0
            if not p.timersActive():                                    # (device form) an inactive row is left alone
                continue
            if p.keepaliveNow:                                          # receive.go:348, owed since finished
                p.keepaliveNow = False
                p.SendKeepalive()
            while True:
                due = [(t.when, i) for i, t in enumerate(p.timers()) if t.isPending and t.when <= self.now]
                if not due:
                    break
                p.timers()[min(due)[1]].callback()
            if p.queued:
                if len(jobs) < n_ka_max:
                    jobs.append(self.peer_id(p))
                    p.acted |= ACT_KEEPALIVE
                else:                                                   # (device form) no room: the next call's
                    p.keepaliveNow = True
                    p.acted |= ACT_DEFERRED
            actions[p.row] = p.acted
        ka_peer = np.full(n_ka_max, PEER_NONE, np.uint32)
        ka_count, ka_sizes, ka_status = (np.zeros(n_ka_max, np.int32) for _ in range(3))
        ka_peer[:len(jobs)], ka_count[:len(jobs)] = jobs, 1
        return dict(ka_peer=ka_peer, ka_count=ka_count, ka_sizes=ka_sizes, ka_status=ka_status,
                    n_ka=np.array([len(jobs)], np.uint32), actions=actions)

    def peer_id(self, p):
        return self.kd.peers[p.row].id

    def render(self):
        out = np.zeros(len(self.by_row), TIMERS_DTYPE)
        for p in self.by_row:
            t = p.timers()
            flags = (p.other_flags | (ACTIVE if p.isRunning else 0) | (NEED_ANOTHER if p.needAnotherKeepalive else 0) |
                     (CLEAR_SRC if p.clearSrc else 0) | (KEEPALIVE_NOW if p.keepaliveNow else 0))
            out[p.row] = ([x.when for x in t], p.lastHandshake,
                          p.other_pending | sum(1 << i for i, x in enumerate(t) if x.isPending), p.handshakeAttempts, flags,
                          p.keepaliveInterval)
        return out
