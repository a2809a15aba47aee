// cs_plan_host.cpp -- the checksum kernel's per-packet plan
// (wireguard_amd/csrc/wgcs_cs_plan.h) as a stand-alone host program, built
// with -fsanitize=address,undefined by tests/test_cs_plan_host.py.
//
// It walks a packet exactly as a row of G lanes of checksum_batch_kernel does
// -- cs_geom() from the descriptor, cs_plan() from the packet's address, every
// lane's edge chunks with their masks, the interior chunks slot by slot, the
// per-lane folds, the parity swap and the pseudo-header term -- over a byte
// buffer, with the header's own functions, and compares the 16-bit result with
// a per-byte RFC 1071 sum written here.  It also checks that every chunk the
// walk touches lies inside the packet's chunk grid, holds a byte that is
// summed, and is read once.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../wireguard_amd/csrc/wgcs_cs_plan.h"

using namespace wgcs;

static int g_fail = 0;
#define CHECK(c, ...)                            \
  do {                                           \
    if (!(c)) {                                  \
      if (++g_fail < 20) {                       \
        printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        printf(__VA_ARGS__);                     \
        printf("\n");                            \
      }                                          \
    }                                            \
  } while (0)

static uint32_t fold32_16(uint32_t x) {
  uint32_t f = (x >> 16) + (x & 0xFFFFu);
  return (f >> 16) + (f & 0xFFFFu);
}
static uint32_t fold64_16(uint64_t x) {
  uint64_t t = (x & 0xFFFFFFFFull) + (x >> 32);
  uint32_t t32 = (uint32_t)(t & 0xFFFFFFFFull) + (uint32_t)(t >> 32);
  return fold32_16(t32);
}
static uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
static uint32_t rotl8(uint32_t x) { return (x << 8) | (x >> 24); }
static uint32_t add_halves(uint32_t acc, uint32_t w) { return acc + (w & 0xFFFFu) + (w >> 16); }
// the kernel's v_perm_b32 selector: byte j of w where bit j of nib is set
static uint32_t keep_bytes(uint32_t w, uint32_t nib) {
  const uint32_t sel = ((nib * 0x00810204u) & 0x04040404u) | 0x03020100u;
  uint32_t r = 0;
  for (int j = 0; j < 4; ++j) {
    const uint32_t s = (sel >> (8 * j)) & 0xFFu;
    if (s >= 4) r |= ((w >> (8 * (s - 4))) & 0xFFu) << (8 * j);
  }
  return r;
}

struct Mem {
  // the packet starts at address kBase + align; mem[0] is address kBase - kBefore
  static constexpr uint32_t kBase = 0x40001000u;
  static constexpr int kBefore = 256;
  std::vector<uint8_t> bytes;
  std::vector<uint8_t> reads;  // per 16-byte chunk address: times read
  uint32_t pbase;
  Mem(int align, int len, uint32_t seed) : bytes(kBefore + 128 + len + 256), pbase(kBase + (uint32_t)align) {
    uint32_t x = seed * 2654435761u + 12345u;
    for (auto& b : bytes) {
      x = x * 1664525u + 1013904223u;
      b = (uint8_t)(x >> 24);
    }
    reads.assign(bytes.size() / 16 + 2, 0);
  }
  size_t at(int pos) const { return (size_t)((int64_t)(pbase - kBase) + kBefore + pos); }
  uint8_t byte(int pos) const { return bytes.at(at(pos)); }
  // one 16-byte chunk load at packet position pos (the address is 16-byte aligned)
  void chunk(int pos, uint32_t w[4]) {
    const size_t a = at(pos);
    CHECK(((pbase + (uint32_t)pos) & 15u) == 0, "unaligned chunk pos %d", pos);
    CHECK(a + 16 <= bytes.size(), "chunk past the buffer pos %d", pos);
    reads.at((a + (kBase - kBefore) % 16) / 16)++;
    for (int k = 0; k < 4; ++k) memcpy(&w[k], &bytes.at(a + 4 * k), 4);
  }
};

struct Case {
  int mode, len, cs, co, proto, v6, align;
  uint32_t amask;
  uint64_t initial;
};

// per-byte reference: checksum(b, init) of RFC 1071 as S == 0 ? 0 : 1 + (S - 1) % 0xFFFF
static uint32_t ref_fold(uint64_t s) { return s == 0 ? 0u : (uint32_t)(1 + (s - 1) % 0xFFFFu); }
static uint64_t ref_words(const Mem& m, int lo, int hi, int fld) {
  uint64_t s = 0;
  for (int i = lo; i < hi; ++i) {
    const uint32_t b = (i == fld || i == fld + 1) ? 0u : m.byte(i);
    s += ((i - lo) & 1) ? b : (b << 8);
  }
  return s;
}
static uint32_t reference(const Mem& m, const Case& c, bool* writes_field) {
  const int fld = (c.cs + c.co) & 0xFFFF;
  *writes_field = false;
  switch (c.mode) {
    case WGCS_MODE_FOLD:
      return ref_fold(ref_words(m, 0, c.len, kCsNoField) + fold64_16(c.initial));
    case WGCS_MODE_L4_FILL:
    case WGCS_MODE_VALIDATE: {
      if (c.cs > c.len) return 0;
      const int f = c.mode == WGCS_MODE_L4_FILL ? fld : kCsNoField;
      const uint64_t s = ref_words(m, c.cs, c.len, f) + ref_words(m, c.v6 ? 8 : 12, c.v6 ? 40 : 20, f) +
                         (uint64_t)c.proto + (uint64_t)((c.len - c.cs) & 0xFFFF);
      const uint32_t t = ref_fold(s);
      if (c.mode == WGCS_MODE_VALIDATE) return t == 0xFFFFu ? 1u : 0u;
      *writes_field = fld + 1 < c.len;
      return (~t) & 0xFFFFu;
    }
    case WGCS_MODE_PARTIAL: {
      const int lo = c.cs < c.len ? c.cs : c.len;
      uint64_t init = 0;
      if (fld + 1 < c.len) init = ((uint32_t)m.byte(fld) << 8) | m.byte(fld + 1);
      return (~ref_fold(ref_words(m, lo, c.len, fld) + init)) & 0xFFFFu;
    }
    default: {  // IP4HDR
      const int hi = c.cs < c.len ? c.cs : c.len;
      return (~ref_fold(ref_words(m, 0, hi, 10))) & 0xFFFFu;
    }
  }
}

// the kernel's walk of one packet by a row of G lanes with U slots
static uint32_t walk(Mem& m, const Case& c, int G, int U) {
  const uint32_t cs_word = (uint32_t)c.cs | ((uint32_t)c.co << 16);
  const CsGeom g = cs_geom(c.mode, true, (uint32_t)c.len, cs_word, (uint32_t)c.proto, c.v6 ? WGCS_PKT_V6 : 0u);
  const CsPlan p = cs_plan(g, m.pbase, c.amask);
  const bool contig = cs_geom_contiguous(g);
  const int head = g.lo_all - p.rel0, end = g.hi_all - p.rel0;
  CHECK(head >= 0 && head <= (int)c.amask, "head %d", head);
  CHECK(((m.pbase + (uint32_t)p.rel0) & c.amask) == 0, "origin not aligned");
  CHECK(p.c_lo >= 0 && p.c_lo <= p.c_hi && p.c_hi <= p.nch && p.nch - p.c_hi <= 1, "counts %d %d %d", p.c_lo, p.c_hi, p.nch);
  CHECK(p.c_lo < (1 << 13), "c_lo %d", p.c_lo);
  const int c_it = cs_first_it(p.c_lo, cs_it_mask(c.amask));
  CHECK(c_it <= p.c_lo && p.c_lo - c_it < 8, "c_it %d c_lo %d", c_it, p.c_lo);
  auto in_grid = [&](int ci, bool interior) {
    const int pos = p.rel0 + 16 * ci;
    CHECK(pos >= p.rel0 && pos + 15 <= g.hi_all + 15 && pos < g.hi_all, "chunk %d outside [rel0, hi_all + 15]", ci);
    CHECK(pos + 16 > g.lo_all, "chunk %d before the first summed byte", ci);
    if (interior) CHECK(pos >= g.hole_end && pos + 16 <= g.hi_all, "interior chunk %d needs a mask", ci);
  };
  uint32_t total = 0;
  for (int sub = 0; sub < G; ++sub) {
    uint32_t acc = 0;
    // edge chunks
    for (int e = sub; e < p.n_edge || e == sub; e += G) {
      const int ce = cs_edge_chunk_index(e, p.c_lo, p.c_hi);
      const bool loaded = e < p.n_edge && cs_edge_loaded(ce, head);
      uint32_t w[4] = {0xDEADBEEFu, 0xA5A5A5A5u, 0xFFFFFFFFu, 0x12345678u};  // not loaded: any value
      if (loaded) {
        in_grid(ce, false);
        m.chunk(p.rel0 + 16 * ce, w);
      }
      if (contig) {
        CHECK(e == sub, "a contiguous range has at most 9 edge chunks");
        const uint32_t m16 = cs_contig_mask16(ce, head, end);
        CHECK(m16 <= 0xFFFFu, "mask %x", m16);
        if (!loaded) CHECK(m16 == 0, "lane %d holds no edge chunk but mask %x", sub, m16);
        for (int k = 0; k < 4; ++k) acc = add_halves(acc, keep_bytes(w[k], (m16 >> (4 * k)) & 0xFu));
      } else if (e < p.n_edge) {
        const int pos = p.rel0 + 16 * ce;
        const uint32_t m16 = cs_main_mask16(g, pos), a16 = cs_addr_mask16(g, pos);
        if (!loaded) CHECK(m16 == 0 && a16 == 0, "edge chunk %d not loaded but masked %x %x", ce, m16, a16);
        for (int k = 0; k < 4; ++k) acc = add_halves(acc, keep_bytes(w[k], (m16 >> (4 * k)) & 0xFu));
        for (int k = 0; k < 4; ++k) {
          uint32_t y = keep_bytes(w[k], (a16 >> (4 * k)) & 0xFu);
          if (p.rot_addr) y = rotl8(y);
          acc = add_halves(acc, y);
        }
      }
    }
    // interior chunks
    bool first = true;
    for (int c0 = c_it + sub; c0 < p.c_hi || first; c0 += G * U) {
      if (!first) acc = (acc >> 16) + (acc & 0xFFFFu);
      first = false;
      const int left = p.c_hi - c0;
      for (int u = 0; u < U; ++u) {
        const bool ok = u * G < left && (u > 0 || c0 >= p.c_lo);
        const int ci = c0 + u * G;
        CHECK(ok == (ci >= p.c_lo && ci < p.c_hi), "slot predicate c %d", ci);
        uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (ok) {
          in_grid(ci, true);
          m.chunk(p.rel0 + 16 * ci, w);
        }
        const uint32_t wt = ok ? 1u : 0u;
        for (int k = 0; k < 4; ++k) acc += wt * ((w[k] & 0xFFFFu) + (w[k] >> 16));
      }
    }
    total += fold32_16(acc);
  }
  for (size_t i = 0; i < m.reads.size(); ++i) CHECK(m.reads[i] <= 1, "chunk read %d times", (int)m.reads[i]);
  uint32_t s = fold32_16(total);
  if (p.swap) s = bswap16(s);
  uint64_t init = 0;
  if (c.mode == WGCS_MODE_FOLD) init = c.initial;
  if (c.mode == WGCS_MODE_PARTIAL && g.fld + 1 < g.main_hi) init = ((uint32_t)m.byte(g.fld) << 8) | m.byte(g.fld + 1);
  const uint32_t t = fold32_16(s + g.pre + fold64_16(init));
  if (c.mode == WGCS_MODE_VALIDATE) return (t == 0xFFFFu && !g.past) ? 1u : 0u;
  if (c.mode == WGCS_MODE_FOLD) return t;
  return g.past ? 0u : ((~t) & 0xFFFFu);
}

static long g_cases = 0;
static void run(const Case& c, int G, int U) {
  Mem m(c.align, c.len, (uint32_t)(c.len * 131 + c.align * 7 + c.mode));
  // make VALIDATE see valid packets too: fix up the checksum field of every other case
  bool wf;
  if (c.mode == WGCS_MODE_VALIDATE && ((c.len + c.align) & 1) && c.cs + 2 <= c.len && c.cs >= (c.v6 ? 40 : 20)) {
    Case f = c;
    f.mode = WGCS_MODE_L4_FILL;
    f.co = 0;
    const uint32_t v = reference(m, f, &wf);
    m.bytes.at(m.at(c.cs)) = (uint8_t)(v >> 8);
    m.bytes.at(m.at(c.cs + 1)) = (uint8_t)v;
    CHECK(reference(m, c, &wf) == 1u, "fix-up did not validate len %d cs %d", c.len, c.cs);
  }
  const uint32_t want = reference(m, c, &wf);
  const uint32_t got = walk(m, c, G, U);
  ++g_cases;
  CHECK(got == want, "mode %d len %d cs %d co %d v6 %d align %d amask %u G %d: got %04x want %04x", c.mode, c.len, c.cs,
        c.co, c.v6, c.align, c.amask, G, got, want);
  // an inactive row sums and reads nothing
  if (c.align == 0 && c.amask == 15) {
    const CsGeom g = cs_geom(c.mode, false, (uint32_t)c.len, (uint32_t)c.cs | ((uint32_t)c.co << 16), (uint32_t)c.proto, 0);
    const CsPlan p = cs_plan(g, m.pbase, 127);
    CHECK(p.nch == 0 && p.n_edge == 0 && p.c_hi == 0, "inactive row has chunks");
  }
}

struct Variant {
  int v6, cs, co_kind;  // cs < 0: len + cs + 1 .. (-1: equal to len, -5: above... see below)
};

static int pick_co(int kind, int cs, int len) {
  switch (kind) {
    case 0: return 6;                                       // first chunk (UDP)
    case 1: return 16;                                      // TCP
    case 2: return len > cs + 4 ? (len - cs) / 2 : 0;       // a middle chunk
    case 3: return len >= cs + 2 ? len - cs - 2 : 1;        // the last two bytes
    case 4: return (len > cs ? len - cs : 0) + 10;          // past the end
    default: return 0xFFF0;                                 // wraps in 16 bits
  }
}

int main() {
  const int modes[5] = {WGCS_MODE_FOLD, WGCS_MODE_L4_FILL, WGCS_MODE_VALIDATE, WGCS_MODE_PARTIAL, WGCS_MODE_IP4HDR};
  // csum_start: the usual header lengths, with options, odd, zero, equal to len (-1), below (-3) and above (-2: len + 4)
  const int v4cs[] = {20, 24, 21, 0, -1, -2, -3};
  const int v6cs[] = {40, 48, 41, -1, -2};
  std::vector<Variant> vars;
  for (int cs : v4cs) vars.push_back({0, cs, 0});
  for (int cs : v6cs) vars.push_back({1, cs, 0});
  auto resolve_cs = [](int cs, int len) { return cs == -1 ? len : cs == -2 ? len + 4 : cs == -3 ? (len > 3 ? len - 3 : 0) : cs; };
  std::vector<int> lens;
  for (int l = 0; l <= 200; ++l) lens.push_back(l);
  for (int l = 1400; l <= 1520; ++l) lens.push_back(l);
  const int sweep[] = {0, 1, 2, 19, 20, 21, 39, 40, 41, 47, 48, 64, 141, 200, 1400, 1499, 1500, 1520};
  // every length x alignment x amask x mode, the variants and field places cycling
  long k = 0;
  for (int mode : modes)
    for (int len : lens)
      for (int align = 0; align < 128; ++align)
        for (uint32_t amask : {15u, 127u}) {
          const Variant& v = vars[(size_t)(k % (long)vars.size())];
          const int cs = resolve_cs(v.cs, len);
          Case c = {mode, len, cs, pick_co((int)(k % 6), cs, len), (k & 1) ? 17 : 6, v.v6, align, amask,
                    0x9E3779B97F4A7C15ull * (uint64_t)(k + 1)};
          if (k % 5 == 0) c.initial = 0;
          run(c, 32, 4);
          ++k;
        }
  // every variant x field place x every third alignment on the lengths where paths change; all lane widths
  for (int mode : modes)
    for (int len : sweep)
      for (const Variant& v : vars)
        for (int ck = 0; ck < 6; ++ck)
          for (int align = ck % 3; align < 128; align += 3) {
            const int cs = resolve_cs(v.cs, len);
            const uint32_t amask = (align ^ ck) & 1 ? 15u : 127u;
            Case c = {mode, len, cs, pick_co(ck, cs, len), 6, v.v6, align, amask, (uint64_t)align << 40 | 0xFFFFFFFFull};
            run(c, 32, 4);
            if (align % 5 == 0) {
              run(c, 16, 4);
              run(c, 64, 2);
              run(c, 16, 8);
            }
          }
  // long packets: several interior iterations, the 16-bit limits of the descriptor fields
  for (int mode : modes)
    for (int len : {2047, 2048, 2049, 9000, 65535, 70000})
      for (int align : {0, 1, 15, 16, 77, 127})
        for (uint32_t amask : {15u, 127u}) {
          run({mode, len, 20, 16, 6, 0, align, amask, 1}, 32, 4);
          run({mode, len, 40, 0xFFFF, 17, 1, align, amask, ~0ull}, 32, 4);
          run({mode, len, 65535, 65535, 17, 0, align, amask, 0}, 32, 4);
          run({mode, len, 20, len - 22, 6, 0, align, amask, 0}, 16, 4);
        }
  printf("%ld cases, %d failures\n", g_cases, g_fail);
  if (g_fail) return 1;
  printf("cs_plan_host: ok\n");
  return 0;
}
