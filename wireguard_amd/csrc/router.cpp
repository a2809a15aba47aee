// router.cpp -- the allowed-IPs trie of device/router.go and the receiver-index
// table of device/sessions.go behind the C ABI (include/wgcsum.h):
//   wgcs_router_insert            Router.Insert, parent.insert     router.go:160-270, :411-424
//   wgcs_router_remove            Router.Remove, node.remove       :272-372, :439-457
//   wgcs_router_remove_by_peer    Router.RemoveByPeer              :460-478
//   wgcs_router_find              Router.Find, node.find           :374-403, :426-437
//   wgcs_router_peer_prefixes     Router.PeerNodes                 :481-495
//   wgcs_router_write_image / wgcs_router_image_find   the flat image the kernels walk (wgcs_route_walk.h)
//   wgcs_session_table_build      SessionMap.Get as an array       sessions.go:26-30
// Host code only: no context, no device, no HIP call.
//
// The trie is restated with node indices in place of pointers.  The reference's
// parent{child **node, childIndex} becomes (parent node index, childIndex):
// childIndex 2 names the root slot of the node's family (:414), 0 / 1 the
// parent's children[childIndex], which is what the pointer arithmetic of
// :347-351 recovers.  Empty nodes (peer == nil) stay as the reference leaves
// them: a removed node with two children (:278-280) and commonNode (:245-253).
// peer.nodes (a list in insertion order, :141-150) is a sequence number per
// node: PushBack takes the next one.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_route_walk.h"

using namespace wgcs;

static_assert(sizeof(wgcs_session_slot) == 8 && sizeof(wgcs_prefix) == 20, "wgcsum.h layouts");

namespace {

constexpr uint32_t kNil = kRouteNone;
constexpr uint8_t kRootSlot = 2;  // parent.childIndex of a root (:414)

struct Node {
  uint32_t parent = kNil;  // the node whose children[parent_ci] points here; unused for a root
  uint8_t parent_ci = kRootSlot;
  uint32_t children[2] = {kNil, kNil};
  uint8_t cidr = 0;
  uint8_t len = 0;  // len(addr): 4 or 16
  uint8_t addr[16] = {};
  uint32_t peer = WGCS_PEER_NONE;
  uint64_t seq = 0;  // position in peer.nodes; 0: not in a list (peerNode == nil)
  bool live = false;
};

// commonBits, router.go:63-91
uint8_t common_bits(const uint8_t* a, const uint8_t* b, int len) {
  uint32_t wa[4], wb[4];
  route_addr_words(a, len / 4, wa);
  route_addr_words(b, len / 4, wb);
  return (uint8_t)route_common_bits(wa, wb, len / 4);
}

// node.childIndex, :95-97
uint8_t child_index(uint8_t cidr, const uint8_t* ip) { return (ip[cidr / 8] >> (7 - cidr % 8)) & 1; }

// maskSelf, :126-139
void mask(uint8_t* addr, int len, uint8_t cidr) {
  for (int i = 0; i < len; ++i) {
    const int bits = (int)cidr - 8 * i;
    const uint8_t m = bits >= 8 ? 0xFF : bits <= 0 ? 0 : (uint8_t)(0xFF << (8 - bits));
    addr[i] &= m;
  }
}

}  // namespace

struct wgcs_router {
  std::shared_mutex mu;
  std::vector<Node> nodes;
  std::vector<uint32_t> free_nodes;
  uint32_t root[2] = {kNil, kNil};  // IPv4, IPv6
  uint32_t live = 0;
  uint64_t next_seq = 1;

  uint32_t alloc() {
    uint32_t i;
    if (!free_nodes.empty()) {
      i = free_nodes.back();
      free_nodes.pop_back();
    } else {
      i = (uint32_t)nodes.size();
      nodes.emplace_back();
    }
    nodes[i] = Node();
    nodes[i].live = true;
    ++live;
    return i;
  }
  // zeroOutPointers (:152-158): the node leaves the trie
  void release(uint32_t i) {
    nodes[i] = Node();
    free_nodes.push_back(i);
    --live;
  }
  // *p.child of parent{child, childIndex}
  uint32_t& slot(int fam, uint32_t parent, uint8_t ci) { return ci == kRootSlot ? root[fam] : nodes[parent].children[ci]; }

  // nodePlacement, :99-122
  uint32_t placement(uint32_t n, const uint8_t* ip, int len, uint8_t cidr, bool* exact) const {
    uint32_t parent = kNil;
    *exact = false;
    while (n != kNil && nodes[n].cidr <= cidr && common_bits(nodes[n].addr, ip, len) >= nodes[n].cidr) {
      parent = n;
      if (nodes[parent].cidr == cidr) {
        *exact = true;
        return parent;
      }
      n = nodes[n].children[child_index(nodes[n].cidr, ip)];
    }
    return parent;
  }

  uint32_t new_node(const uint8_t* ip, int len, uint8_t cidr, uint32_t peer) {
    const uint32_t i = alloc();
    Node& nd = nodes[i];
    nd.cidr = cidr;
    nd.len = (uint8_t)len;
    memcpy(nd.addr, ip, len);
    mask(nd.addr, len, cidr);
    nd.peer = peer;
    if (peer != WGCS_PEER_NONE) nd.seq = next_seq++;  // addToPeerNodes
    return i;
  }
  void set_parent(uint32_t n, uint32_t parent, uint8_t ci) {
    nodes[n].parent = parent;
    nodes[n].parent_ci = ci;
  }

  // parent.insert, :160-270, with p = the root slot of family fam
  void insert(int fam, const uint8_t* ip, int len, uint8_t cidr, uint32_t peer) {
    if (root[fam] == kNil) {  // CASE 1, :165-179
      const uint32_t nn = new_node(ip, len, cidr, peer);
      set_parent(nn, kNil, kRootSlot);
      root[fam] = nn;
      return;
    }
    bool exact;
    const uint32_t parent = placement(root[fam], ip, len, cidr, &exact);  // :182
    if (exact) {  // CASE 2, :186-191: the prefix moves to the back of the new peer's list
      nodes[parent].peer = peer;
      nodes[parent].seq = next_seq++;
      return;
    }
    const uint32_t nn = new_node(ip, len, cidr, peer);  // :192-200 (may move `nodes`: index, not reference, from here)
    const uint8_t* nip = nodes[nn].addr;                // the reference's ip aliases newNode.addr: masked from here on
    uint32_t down;
    if (parent == kNil) {  // CASE 3, :205-207
      down = root[fam];
    } else {  // CASE 4, :208-220
      const uint8_t index = child_index(nodes[parent].cidr, nip);
      down = nodes[parent].children[index];
      if (down == kNil) {  // CASE 5
        set_parent(nn, parent, index);
        nodes[parent].children[index] = nn;
        return;
      }
    }
    const uint8_t common = common_bits(nodes[down].addr, nip, len);  // :224
    const uint8_t ccidr = std::min(cidr, common);
    if (nodes[nn].cidr == ccidr) {  // CASE 6, :228-242
      const uint8_t index = child_index(nodes[nn].cidr, nodes[down].addr);
      set_parent(down, nn, index);
      nodes[nn].children[index] = down;
      if (parent == kNil) {  // CASE 7
        set_parent(nn, kNil, kRootSlot);
        root[fam] = nn;
      } else {  // CASE 8
        const uint8_t pi = child_index(nodes[parent].cidr, nodes[nn].addr);
        set_parent(nn, parent, pi);
        nodes[parent].children[pi] = nn;
      }
      return;
    }
    uint8_t caddr[16];
    memcpy(caddr, nodes[nn].addr, 16);
    const uint32_t cn = new_node(caddr, len, ccidr, WGCS_PEER_NONE);  // commonNode, :245-254
    uint8_t index = child_index(ccidr, nodes[down].addr);
    set_parent(down, cn, index);
    nodes[cn].children[index] = down;
    index = child_index(ccidr, nodes[nn].addr);
    set_parent(nn, cn, index);
    nodes[cn].children[index] = nn;
    if (parent == kNil) {  // CASE 9
      set_parent(cn, kNil, kRootSlot);
      root[fam] = cn;
    } else {  // CASE 10
      const uint8_t pi = child_index(nodes[parent].cidr, nodes[cn].addr);
      set_parent(cn, parent, pi);
      nodes[parent].children[pi] = cn;
    }
  }

  // node.remove, :273-372
  void remove(int fam, uint32_t n) {
    nodes[n].seq = 0;  // removeFromPeerNodes
    nodes[n].peer = WGCS_PEER_NONE;
    if (nodes[n].children[0] != kNil && nodes[n].children[1] != kNil) return;  // :278-280: stays, empty
    const int index = nodes[n].children[0] == kNil ? 1 : 0;
    uint32_t child = nodes[n].children[index];
    const uint32_t np = nodes[n].parent;
    const uint8_t nci = nodes[n].parent_ci;
    if (child != kNil) set_parent(child, np, nci);  // :289-291
    slot(fam, np, nci) = child;                     // :292
    if (child != kNil || nci > 1) {                 // :296-299
      release(n);
      return;
    }
    const uint32_t parent = np;  // :347-351
    if (nodes[parent].peer != WGCS_PEER_NONE) {  // :354-357
      release(n);
      return;
    }
    child = nodes[parent].children[nci ^ 1];  // :359
    const uint32_t pp = nodes[parent].parent;
    const uint8_t pci = nodes[parent].parent_ci;
    if (child != kNil) set_parent(child, pp, pci);  // :366-368
    slot(fam, pp, pci) = child;                     // :369
    release(n);
    release(parent);
  }

  // node.find, :374-403
  uint32_t find(uint32_t n, const uint8_t* ip, int len) const {
    uint32_t peer = WGCS_PEER_NONE;
    while (n != kNil && common_bits(nodes[n].addr, ip, len) >= nodes[n].cidr) {
      if (nodes[n].peer != WGCS_PEER_NONE) peer = nodes[n].peer;
      if (nodes[n].cidr / 8 == len) break;  // n.index == ipLen
      n = nodes[n].children[child_index(nodes[n].cidr, ip)];
    }
    return peer;
  }

  // the nodes of peer.nodes, front to back
  std::vector<uint32_t> peer_nodes(uint32_t peer) const {
    std::vector<uint32_t> v;
    for (uint32_t i = 0; i < nodes.size(); ++i)
      if (nodes[i].live && nodes[i].peer == peer && nodes[i].seq) v.push_back(i);
    std::sort(v.begin(), v.end(), [&](uint32_t a, uint32_t b) { return nodes[a].seq < nodes[b].seq; });
    return v;
  }
  int family_of(uint32_t n) const { return nodes[n].len == 16; }
};

namespace {

bool good_len(size_t addr_len) { return addr_len == 4 || addr_len == 16; }

}  // namespace

extern "C" {

wgcs_router* wgcs_router_create(void) { return new (std::nothrow) wgcs_router(); }

void wgcs_router_destroy(wgcs_router* r) { delete r; }

int wgcs_router_insert(wgcs_router* r, const uint8_t* addr, size_t addr_len, uint8_t cidr, uint32_t peer) {
  if (!r || !addr || !good_len(addr_len) || cidr > 8 * addr_len || peer == WGCS_PEER_NONE) return WGCS_ERR_INVALID_ARG;
  std::unique_lock<std::shared_mutex> g(r->mu);
  try {
    // an insert makes at most two nodes: with room for them nothing throws half-way
    if (r->nodes.capacity() < r->nodes.size() + 2) r->nodes.reserve(std::max<size_t>(16, 2 * r->nodes.capacity()));
    r->free_nodes.reserve(r->nodes.capacity());
  } catch (const std::bad_alloc&) {
    return WGCS_ERR_NOMEM;
  }
  r->insert(addr_len == 16, addr, (int)addr_len, cidr, peer);
  return WGCS_OK;
}

int wgcs_router_remove(wgcs_router* r, const uint8_t* addr, size_t addr_len, uint8_t cidr, uint32_t peer) {
  if (!r || !addr || !good_len(addr_len) || cidr > 8 * addr_len) return WGCS_ERR_INVALID_ARG;
  std::unique_lock<std::shared_mutex> g(r->mu);
  const int fam = addr_len == 16;
  bool exact;
  const uint32_t n = r->placement(r->root[fam], addr, (int)addr_len, cidr, &exact);  // :444-452
  if (n == kNil || !exact || peer != r->nodes[n].peer) return WGCS_OK;               // :453-455
  r->remove(fam, n);
  return WGCS_OK;
}

int wgcs_router_remove_by_peer(wgcs_router* r, uint32_t peer) {
  if (!r) return WGCS_ERR_INVALID_ARG;
  if (peer == WGCS_PEER_NONE) return WGCS_OK;  // no node is in nil's list
  std::unique_lock<std::shared_mutex> g(r->mu);
  try {
    // removing one node of the list frees that node and at most its empty
    // parent, never another element of the list (:472-477)
    for (uint32_t n : r->peer_nodes(peer)) r->remove(r->family_of(n), n);
  } catch (const std::bad_alloc&) {
    return WGCS_ERR_NOMEM;
  }
  return WGCS_OK;
}

uint32_t wgcs_router_find(wgcs_router* r, const uint8_t* addr, size_t addr_len) {
  if (!r || !addr || !good_len(addr_len)) return WGCS_PEER_NONE;
  std::shared_lock<std::shared_mutex> g(r->mu);
  return r->find(r->root[addr_len == 16], addr, (int)addr_len);
}

int wgcs_router_peer_prefixes(wgcs_router* r, uint32_t peer, wgcs_prefix* out, size_t cap, size_t* n) {
  if (!r || !n || (cap && !out)) return WGCS_ERR_INVALID_ARG;
  *n = 0;
  if (peer == WGCS_PEER_NONE) return WGCS_OK;
  std::shared_lock<std::shared_mutex> g(r->mu);
  try {
    const std::vector<uint32_t> v = r->peer_nodes(peer);
    *n = v.size();
    for (size_t k = 0; k < v.size() && k < cap; ++k) {
      const Node& nd = r->nodes[v[k]];
      memset(&out[k], 0, sizeof out[k]);
      out[k].addr_len = r->family_of(v[k]) ? 16 : 4;
      memcpy(out[k].addr, nd.addr, out[k].addr_len);
      out[k].cidr = nd.cidr;
    }
  } catch (const std::bad_alloc&) {
    return WGCS_ERR_NOMEM;
  }
  return WGCS_OK;
}

size_t wgcs_router_image_size(wgcs_router* r) {
  if (!r) return 0;
  std::shared_lock<std::shared_mutex> g(r->mu);
  return kRouteHeaderBytes + (size_t)r->live * kRouteNodeBytes;
}

int wgcs_router_write_image(wgcs_router* r, uint8_t* buf, size_t cap, size_t* len) {
  if (!r || !buf || !len) return WGCS_ERR_INVALID_ARG;
  *len = 0;
  std::shared_lock<std::shared_mutex> g(r->mu);
  const size_t need = kRouteHeaderBytes + (size_t)r->live * kRouteNodeBytes;
  if (cap < need) return WGCS_ERR_OUT_OF_RANGE;
  std::vector<uint32_t> dense;  // node index -> image index
  try {
    dense.assign(r->nodes.size(), kNil);
  } catch (const std::bad_alloc&) {
    return WGCS_ERR_NOMEM;
  }
  uint32_t count = 0;
  for (uint32_t i = 0; i < r->nodes.size(); ++i)
    if (r->nodes[i].live) dense[i] = count++;
  auto at = [&](uint32_t i) { return i == kNil ? kNil : dense[i]; };
  RouteHeader h = {kRouteMagic, kRouteVersion, count, at(r->root[0]), at(r->root[1]), {0, 0, 0}};
  memcpy(buf, &h, sizeof h);
  for (uint32_t i = 0; i < r->nodes.size(); ++i) {
    const Node& nd = r->nodes[i];
    if (!nd.live) continue;
    RouteNode o;
    route_addr_words(nd.addr, 4, o.addr);
    o.child[0] = at(nd.children[0]);
    o.child[1] = at(nd.children[1]);
    o.peer = nd.peer;
    o.cidr = nd.cidr;
    memcpy(buf + kRouteHeaderBytes + (size_t)dense[i] * kRouteNodeBytes, &o, sizeof o);
  }
  *len = need;
  return WGCS_OK;
}

int wgcs_router_image_find(const uint8_t* buf, size_t len, const uint8_t* addr, size_t addr_len, uint32_t* peer) {
  if (!peer) return WGCS_ERR_INVALID_ARG;
  *peer = WGCS_PEER_NONE;
  if (!buf || !addr || !good_len(addr_len)) return WGCS_ERR_INVALID_ARG;
  uint32_t a[4] = {0, 0, 0, 0};
  route_addr_words(addr, (int)addr_len / 4, a);
  return route_image_find(buf, len, a, addr_len == 16, peer);
}

int wgcs_session_table_build(const uint32_t* indices, const uint32_t* keys, uint32_t n, wgcs_session_slot* slots,
                             uint32_t n_slots) {
  if (!slots || (n && (!indices || !keys))) return WGCS_ERR_INVALID_ARG;
  if (n_slots == 0 || (n_slots & (n_slots - 1)) || (uint64_t)n_slots < 2 * (uint64_t)n) return WGCS_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n_slots; ++i) slots[i] = wgcs_session_slot{0, kSessionEmpty};
  const uint32_t mask = n_slots - 1;
  for (uint32_t i = 0; i < n; ++i) {
    if (keys[i] == kSessionEmpty) return WGCS_ERR_INVALID_ARG;
    uint32_t at = session_hash(indices[i]) & mask;
    while (slots[at].key != kSessionEmpty) {  // at least half of the slots are empty: this ends
      if (slots[at].index == indices[i]) return WGCS_ERR_INVALID_ARG;
      at = (at + 1) & mask;
    }
    slots[at] = wgcs_session_slot{indices[i], keys[i]};
  }
  return WGCS_OK;
}

}  // extern "C"
