// route_host.cpp -- the host router (wireguard_amd/csrc/router.cpp) and the
// image walk the kernels run (wgcs_route_walk.h) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_route_host.py builds and runs it):
//   1. random inserts and removes over a small address universe, every lookup
//      checked against a brute-force longest-prefix match kept here;
//   2. the walk on valid images and on damaged ones -- truncated at every
//      length, every 32-bit word of an image overwritten with hostile values
//      (child indices at and past the node count, a node as its own child, a
//      bad magic, a huge node count, cidr out of range): each call must end
//      with a peer or WGCS_PEER_NONE, or with WGCS_ERR_INVALID_ARG, without a
//      sanitizer report and within the visit bound;
//   3. the session slots: every listed index found, others not.
// Damaged images exist only here: none is ever given to a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../../wireguard_amd/csrc/router.cpp"

namespace {

int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      if (fails++ < 20) printf("line %d: %s\n", __LINE__, #c);    \
    }                                                             \
  } while (0)

struct Addr {
  uint8_t b[16];
  int len;
};
using Key = std::tuple<int, std::vector<uint8_t>, int>;  // len, masked address, cidr

std::mt19937 rng(20261019);
uint32_t pick(std::initializer_list<uint32_t> v) { return v.begin()[rng() % v.size()]; }

void rand_prefix(Addr* a, uint8_t* cidr) {
  memset(a->b, 0, 16);
  if (rng() % 5 < 3) {
    a->len = 4;
    a->b[0] = 10;
    a->b[1] = (uint8_t)pick({0, 1, 128});
    a->b[2] = (uint8_t)pick({0, 1});
    a->b[3] = (uint8_t)pick({0, 1, 255});
    *cidr = (uint8_t)pick({0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32});
  } else {
    a->len = 16;
    a->b[0] = 0x20, a->b[1] = 0x01, a->b[2] = 0x0d, a->b[3] = 0xb8;
    a->b[8] = (uint8_t)pick({0, 128});
    a->b[11] = (uint8_t)pick({0, 1});
    a->b[14] = (uint8_t)pick({0, 1});
    a->b[15] = (uint8_t)pick({0, 1, 255});
    *cidr = (uint8_t)pick({0, 1, 32, 63, 64, 65, 96, 97, 120, 127, 128});
  }
}

Key key_of(const Addr& a, int cidr) {
  std::vector<uint8_t> m(a.b, a.b + a.len);
  for (int i = 0; i < a.len; ++i) {
    const int bits = cidr - 8 * i;
    if (bits <= 0) m[i] = 0;
    else if (bits < 8) m[i] &= (uint8_t)(0xFF << (8 - bits));
  }
  return Key(a.len, m, cidr);
}

bool covers(const Key& k, const uint8_t* ip) {
  const std::vector<uint8_t>& m = std::get<1>(k);
  for (int bit = 0; bit < std::get<2>(k); ++bit)
    if (((m[bit / 8] ^ ip[bit / 8]) >> (7 - bit % 8)) & 1) return false;
  return true;
}

uint32_t brute_find(const std::map<Key, uint32_t>& table, const uint8_t* ip, int len) {
  uint32_t best = WGCS_PEER_NONE;
  int best_cidr = -1;
  for (const auto& kv : table)
    if (std::get<0>(kv.first) == len && std::get<2>(kv.first) > best_cidr && covers(kv.first, ip)) {
      best = kv.second;
      best_cidr = std::get<2>(kv.first);
    }
  return best;
}

std::vector<uint8_t> image_of(wgcs_router* r) {
  std::vector<uint8_t> img(wgcs_router_image_size(r));
  size_t len = 0;
  CHECK(wgcs_router_write_image(r, img.data(), img.size(), &len) == WGCS_OK && len == img.size());
  return img;
}

// every prefix's first and last address and their neighbours, three ways
void compare(wgcs_router* r, const std::map<Key, uint32_t>& table) {
  // the image in a heap block of exactly its size: ASan sees any read past it
  const std::vector<uint8_t> img = image_of(r);
  for (const auto& kv : table) {
    const int len = std::get<0>(kv.first), cidr = std::get<2>(kv.first);
    for (int edge = 0; edge < 2; ++edge)
      for (int delta = -1; delta <= 1; ++delta) {
        uint8_t ip[16];
        memcpy(ip, std::get<1>(kv.first).data(), len);
        if (edge)
          for (int bit = cidr; bit < 8 * len; ++bit) ip[bit / 8] |= (uint8_t)(1 << (7 - bit % 8));
        for (int i = len - 1, carry = delta; i >= 0 && carry; --i) {  // ip += delta, wrapping
          const int v = ip[i] + carry;
          ip[i] = (uint8_t)v;
          carry = v < 0 ? -1 : v > 255 ? 1 : 0;
        }
        const uint32_t want = brute_find(table, ip, len);
        CHECK(wgcs_router_find(r, ip, len) == want);
        uint32_t got = 0;
        CHECK(wgcs_router_image_find(img.data(), img.size(), ip, len, &got) == WGCS_OK && got == want);
      }
  }
}

void fuzz_router() {
  wgcs_router* r = wgcs_router_create();
  std::map<Key, uint32_t> table;
  for (int step = 0; step < 2000; ++step) {
    Addr a;
    uint8_t cidr;
    rand_prefix(&a, &cidr);
    const uint32_t peer = 1 + rng() % 4;
    const uint32_t op = rng() % 10;
    if (op < 5 || table.empty()) {
      CHECK(wgcs_router_insert(r, a.b, a.len, cidr, peer) == WGCS_OK);
      table[key_of(a, cidr)] = peer;
    } else if (op < 9) {
      if (rng() % 5) {  // mostly a prefix that is there
        auto it = table.begin();
        std::advance(it, rng() % table.size());
        a.len = std::get<0>(it->first);
        memcpy(a.b, std::get<1>(it->first).data(), a.len);
        cidr = (uint8_t)std::get<2>(it->first);
      }
      auto it = table.find(key_of(a, cidr));
      const uint32_t who = (it != table.end() && rng() % 5) ? it->second : peer;
      CHECK(wgcs_router_remove(r, a.b, a.len, cidr, who) == WGCS_OK);
      if (it != table.end() && it->second == who) table.erase(it);
    } else {
      CHECK(wgcs_router_remove_by_peer(r, peer) == WGCS_OK);
      for (auto it = table.begin(); it != table.end();) it = it->second == peer ? table.erase(it) : std::next(it);
    }
    compare(r, table);
    size_t n = 0, total = 0;
    for (uint32_t p = 1; p <= 4; ++p) {
      CHECK(wgcs_router_peer_prefixes(r, p, nullptr, 0, &n) == WGCS_OK);
      std::vector<wgcs_prefix> out(n);
      CHECK(wgcs_router_peer_prefixes(r, p, out.data(), n, &n) == WGCS_OK && n == out.size());
      total += n;
    }
    CHECK(total == table.size());
  }
  wgcs_router_destroy(r);
}

// One lookup on a possibly damaged image: any answer but a crash, a read
// outside the block or an endless loop is acceptable.
void walk(const std::vector<uint8_t>& img, size_t len) {
  // a block of exactly len bytes, so that a read past a truncated image is a heap overflow ASan reports
  uint8_t* block = (uint8_t*)malloc(len ? len : 1);
  memcpy(block, img.data(), len);
  static const uint8_t probes[][16] = {
      {10, 1, 2, 3}, {10, 128, 0, 1}, {255, 255, 255, 255}, {0},
      {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1}, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff}};
  for (const auto& p : probes)
    for (size_t alen : {(size_t)4, (size_t)16}) {
      uint32_t peer = 12345;
      const int rc = wgcs_router_image_find(block, len, p, alen, &peer);
      CHECK(rc == WGCS_OK || rc == WGCS_ERR_INVALID_ARG);
      CHECK(rc == WGCS_OK || peer == WGCS_PEER_NONE);
    }
  free(block);
}

void damaged_images() {
  wgcs_router* r = wgcs_router_create();
  // chains, so that walks are deep: /1../32 and /1../128 along one address, plus a few branches
  const uint8_t a4[4] = {10, 1, 2, 3};
  uint8_t a6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int c = 0; c <= 32; ++c) CHECK(wgcs_router_insert(r, a4, 4, (uint8_t)c, 1 + c % 3) == WGCS_OK);
  for (int c = 0; c <= 128; ++c) CHECK(wgcs_router_insert(r, a6, 16, (uint8_t)c, 1 + c % 5) == WGCS_OK);
  const uint8_t b4[4] = {10, 128, 0, 0}, c4[4] = {192, 168, 0, 0};
  CHECK(wgcs_router_insert(r, b4, 4, 9, 7) == WGCS_OK && wgcs_router_insert(r, c4, 4, 16, 8) == WGCS_OK);
  const std::vector<uint8_t> img = image_of(r);
  const uint32_t n_nodes = (uint32_t)((img.size() - kRouteHeaderBytes) / kRouteNodeBytes);
  CHECK(n_nodes >= 33 + 129);
  uint32_t peer = 0;
  CHECK(wgcs_router_image_find(img.data(), img.size(), a4, 4, &peer) == WGCS_OK && peer == 1 + 32 % 3);
  CHECK(wgcs_router_image_find(img.data(), img.size(), a6, 16, &peer) == WGCS_OK && peer == 1 + 128 % 5);  // 129 visits

  for (size_t len = 0; len <= img.size(); ++len) walk(img, len);  // truncated everywhere

  // a header that promises more nodes than the bytes hold, and a bad magic / version
  const uint32_t hostile[] = {0, 1, n_nodes - 1, n_nodes, n_nodes + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu,
                              33, 128, 129, 255, 256};
  for (size_t word = 0; word < img.size() / 4; ++word)
    for (uint32_t v : hostile) {
      std::vector<uint8_t> bad = img;
      memcpy(&bad[4 * word], &v, 4);
      walk(bad, bad.size());
    }
  {
    std::vector<uint8_t> bad = img;
    bad[0] ^= 1;  // magic
    CHECK(wgcs_router_image_find(bad.data(), bad.size(), a4, 4, &peer) == WGCS_ERR_INVALID_ARG && peer == WGCS_PEER_NONE);
    bad = img;
    bad[4] ^= 3;  // version
    CHECK(wgcs_router_image_find(bad.data(), bad.size(), a4, 4, &peer) == WGCS_ERR_INVALID_ARG);
    bad = img;
    const uint32_t more = n_nodes + 1;  // one node more than the bytes hold
    memcpy(&bad[8], &more, 4);
    CHECK(wgcs_router_image_find(bad.data(), bad.size(), a4, 4, &peer) == WGCS_ERR_INVALID_ARG);
  }
  // every node made its own child on both sides, and every child index at / past the node count
  for (uint32_t v : {0u, 1u, 2u}) {
    std::vector<uint8_t> bad = img;
    for (uint32_t i = 0; i < n_nodes; ++i) {
      const uint32_t idx = v == 0 ? i : v == 1 ? n_nodes : n_nodes + 1000u + i;
      memcpy(&bad[kRouteHeaderBytes + i * kRouteNodeBytes + 16], &idx, 4);
      memcpy(&bad[kRouteHeaderBytes + i * kRouteNodeBytes + 20], &idx, 4);
    }
    walk(bad, bad.size());
    CHECK(wgcs_router_image_find(bad.data(), bad.size(), a6, 16, &peer) == WGCS_ERR_INVALID_ARG && peer == WGCS_PEER_NONE);
  }
  // a cycle of two nodes whose cidr does not rise is cut by the rising-cidr rule, not by luck
  {
    std::vector<uint8_t> two(kRouteHeaderBytes + 2 * kRouteNodeBytes, 0);
    RouteHeader h = {kRouteMagic, kRouteVersion, 2, 0, kRouteNone, {0, 0, 0}};
    memcpy(two.data(), &h, sizeof h);
    RouteNode n0 = {{0, 0, 0, 0}, {1, 1}, 5, 0}, n1 = {{0, 0, 0, 0}, {0, 0}, 6, 0};
    memcpy(&two[kRouteHeaderBytes], &n0, sizeof n0);
    memcpy(&two[kRouteHeaderBytes + kRouteNodeBytes], &n1, sizeof n1);
    CHECK(wgcs_router_image_find(two.data(), two.size(), a4, 4, &peer) == WGCS_ERR_INVALID_ARG && peer == WGCS_PEER_NONE);
  }
  wgcs_router_destroy(r);
}

void sessions() {
  for (uint32_t n : {0u, 1u, 64u, 1000u}) {
    uint32_t n_slots = 1;
    while (n_slots < 2 * n) n_slots *= 2;
    std::vector<uint32_t> idx(n), key(n);
    std::map<uint32_t, uint32_t> want;
    for (uint32_t i = 0; i < n; ++i) {
      do idx[i] = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : (n == 1000 ? i * 2048u : (uint32_t)rng());
      while (want.count(idx[i]));
      key[i] = i;
      want[idx[i]] = i;
    }
    std::vector<wgcs_session_slot> slots(n_slots);
    CHECK(wgcs_session_table_build(idx.data(), key.data(), n, slots.data(), n_slots) == WGCS_OK);
    for (const auto& kv : want) CHECK(session_get(slots.data(), n_slots, kv.first) == kv.second);
    for (int k = 0; k < 2000; ++k) {
      const uint32_t x = (uint32_t)rng();
      CHECK(session_get(slots.data(), n_slots, x) == (want.count(x) ? want[x] : kSessionEmpty));
    }
    if (n) CHECK(wgcs_session_table_build(idx.data(), key.data(), n, slots.data(), n_slots / 2) == WGCS_ERR_INVALID_ARG);
    // a table with no empty slot (not one build makes): the probe still ends
    std::vector<wgcs_session_slot> full(8, wgcs_session_slot{1, 1});
    CHECK(session_get(full.data(), 8, 2) == kSessionEmpty);
  }
}

}  // namespace

int main() {
  fuzz_router();
  damaged_images();
  sessions();
  if (fails) {
    printf("route_host: %d checks failed\n", fails);
    return 1;
  }
  printf("route_host: ok\n");
  return 0;
}
