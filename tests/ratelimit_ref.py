"""A literal restatement of the reference's rate limiter, as plain Python over
objects (test infrastructure; never on a hot path):

  RateLimiter.Allow     ratelimiter/ratelimiter.go:91-126
  RateLimiter.cleanup   ratelimiter.go:77-89
  RateLimiter.batch     the rows of a receive batch, Allow called once per row in
                        row order, as RoutineHandshake does for each message that
                        passed the screen under load       device/receive.go:283-286

The table is a dict from a netip.Addr stand-in, (family, the address bytes
padded to 16), to an Entry; the clock is injected: r.now() reads RateLimiter.now_ns,
which a batch holds still.  Nothing here knows a closed form: every row is one
Allow.

What the device form adds to the reference is restated here too, and marked:
  * the table is bounded: with `capacity` entries in it a new address is refused
    with ERR_RATE_TABLE_FULL and leaves no entry;
  * the ticker is the caller's: cleanup() is called by the test.
"""
HS_PASS = 1
ERR_INVALID_ARG, ERR_RATE_LIMITED, ERR_RATE_TABLE_FULL = -1, -28, -29

packetsPerSecond = 20
packetCost = 1_000_000_000 // packetsPerSecond   # :14
packetsBurst = 5
maxTokens = packetCost * packetsBurst            # :19
cleanupInterval = 1_000_000_000                  # :21


class Entry:
    def __init__(self):
        self.tokens = 0
        self.lastTime = 0


class TableFull(Exception):
    pass


def addr_of(src_row):
    """The netip.Addr of one SRC_ADDR_DTYPE row, or None for a bad len."""
    n = int(src_row["len"])
    if n not in (6, 18):
        return None
    ip = bytes(src_row["b"][:n - 2])
    return (len(ip), ip + bytes(16 - len(ip)))


class RateLimiter:
    def __init__(self, capacity=None):
        self.table = {}
        self.now_ns = 0
        self.capacity = capacity  # marked: the bounded table

    def now(self):
        return self.now_ns

    def cleanup(self):  # :77-89
        for k in list(self.table):
            v = self.table[k]
            if self.now() - v.lastTime > cleanupInterval:
                del self.table[k]
        return len(self.table) == 0

    def Allow(self, ip):  # :91-126
        entry = self.table.get(ip)
        if entry is None:
            if self.capacity is not None and len(self.table) >= self.capacity:  # marked
                raise TableFull
            entry = Entry()
            entry.tokens = maxTokens - packetCost
            entry.lastTime = self.now()
            self.table[ip] = entry
            return True
        now = self.now()
        entry.tokens += now - entry.lastTime
        entry.lastTime = now
        entry.tokens = min(entry.tokens, maxTokens)
        if entry.tokens >= packetCost:
            entry.tokens -= packetCost
            return True
        return False

    def batch(self, gate, src, now_ns):
        """The verdicts of the rows, and {passed, limited, table_full, entries_created}."""
        self.now_ns = now_ns
        verdict, stats = [], [0, 0, 0, 0]
        for g, s in zip(gate, src):
            if int(g) != HS_PASS:
                verdict.append(int(g))
                continue
            ip = addr_of(s)
            if ip is None:
                verdict.append(ERR_INVALID_ARG)
                continue
            before = len(self.table)
            try:
                ok = self.Allow(ip)
            except TableFull:
                verdict.append(ERR_RATE_TABLE_FULL)
                stats[2] += 1
                continue
            stats[3] += len(self.table) - before
            stats[0 if ok else 1] += 1
            verdict.append(HS_PASS if ok else ERR_RATE_LIMITED)
        return verdict, stats

    def entries(self):
        return {k: (v.tokens, v.lastTime) for k, v in self.table.items()}
