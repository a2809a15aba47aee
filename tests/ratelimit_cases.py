"""Shared by the rate limiter's tests: source rows, addresses that collide in a
table, and the check that a table is one the probe can read."""
import ipaddress

import numpy as np

from wireguard_amd import ratelimit as rl
from wireguard_amd.cookie import SRC_ADDR_DTYPE, src_addr

HS_NONE, HS_PASS, HS_COOKIE, ERR_MAC1 = 0, 1, 2, -21
COST, MAX, SECOND = rl.RL_PACKET_COST_NS, rl.RL_MAX_TOKENS_NS, 1_000_000_000


def srcs(addrs) -> np.ndarray:
    """SRC_ADDR_DTYPE rows of (ip, port) pairs; ip a string or 4 / 16 bytes."""
    out = np.zeros(len(addrs), SRC_ADDR_DTYPE)
    for i, (ip, port) in enumerate(addrs):
        out[i] = src_addr(ip, port)[0]
    return out


def v4(i: int) -> str:
    return str(ipaddress.IPv4Address(0x0A000000 + i))


def key_of(ip) -> tuple:
    a = ipaddress.ip_address(ip).packed if isinstance(ip, str) else bytes(ip)
    return (len(a), a + bytes(16 - len(a)))


_homes = {}


def home_of(i: int, n_slots: int) -> int:
    """The home slot of v4(i), asked of the library's export once."""
    if (i, n_slots) not in _homes:
        _homes[i, n_slots] = rl.home_slot(src_addr(v4(i), 1), n_slots)
    return _homes[i, n_slots]


def colliding(n_slots: int, home: int, count: int, start: int = 0) -> list:
    """`count` IPv4 addresses (strings) whose home slot in a table of n_slots
    is `home`, found through the library's export."""
    out, i = [], start
    while len(out) < count:
        if home_of(i, n_slots) == home:
            out.append(v4(i))
        i += 1
    return out


def by_home(n_slots: int, homes, start: int = 0) -> list:
    """One IPv4 address per entry of `homes`, with that home slot, all different."""
    out, used = [], set()
    for h in homes:
        i = start
        while i in used or home_of(i, n_slots) != h:
            i += 1
        used.add(i)
        out.append(v4(i))
    return out


def distinct_homes(n_slots: int, count: int) -> list:
    """`count` (home, IPv4 address) pairs in ascending order of home, no home
    twice: in an empty table every one of them lands in its home slot, so the
    key order of a batch over them is this order."""
    seen, i = {}, 0
    while len(seen) < count:
        seen.setdefault(home_of(i, n_slots), v4(i))
        i += 1
    return sorted(seen.items())


def check_reachable(tab) -> None:
    """Every row is empty or live, and every live row is reached by the probe
    from its home slot with no empty slot on the way."""
    if hasattr(tab, "cpu"):
        tab = tab.cpu().numpy()
    t = np.ascontiguousarray(tab).reshape(-1).view(np.uint8).view(rl.RL_ENTRY_DTYPE)
    n = len(t)
    assert set(np.unique(t["state"]).tolist()) <= {0, 1}
    empty = t[t["state"] == 0]
    assert not empty.view(np.uint8).any(), "an empty row is all zero"
    for i in np.flatnonzero(t["state"] == 1):
        fam = int(t["family"][i])
        assert fam in (4, 16) and (fam == 16 or not t["ip"][i][4:].any())
        s = rl.home_slot(src_addr(t["ip"][i][:fam].tobytes(), 0), n)
        while s != i:
            assert t["state"][s] == 1, f"slot {s} is empty between home and slot {i}"
            s = (s + 1) % n
